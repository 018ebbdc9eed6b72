!! ISO_C_BINDING view of include/athena_mp.h -- the thin shim the north star asks for.
!! Every interface is `bind(C)`; the ones invoked from diffstruc's `pure` get_partial_*_val
!! callbacks are declared `pure` (legal for bind(C) interfaces; SURVEY.md 8b).
!! Host arrays are passed by reference exactly as Fortran holds them: array_type%val(F,N) is
!! column-major, i.e. the row-major [N][F] the kernels read; adj_ia / adj_ja keep their 1-based
!! values (athena_mp_graph_create converts once).
module athena_mp_c
  use, intrinsic :: iso_c_binding
  implicit none
  private

  integer(c_int), parameter, public :: ATHENA_MP_ACT_NONE = 0, ATHENA_MP_ACT_RELU = 1, &
       ATHENA_MP_ACT_SIGMOID = 2, ATHENA_MP_ACT_TANH = 3

  public :: athena_mp_init, athena_mp_initialized, athena_mp_finalize, athena_mp_last_error, athena_mp_synchronize
  public :: athena_mp_graph_create, athena_mp_graph_destroy, athena_mp_graph_key
  public :: athena_mp_graph_acquire, athena_mp_graph_release, athena_mp_graph_evict, athena_mp_graph_cache_stats
  public :: athena_mp_kipf_propagate_fwd_host, athena_mp_kipf_propagate_bwd_host
  public :: athena_mp_gemm_fwd_host
  public :: athena_mp_duvenaud_propagate_fwd_host, athena_mp_duvenaud_propagate_bwd_x_host
  public :: athena_mp_duvenaud_update_fwd_host
  public :: athena_mp_duvenaud_propagate_bwd_e_host, athena_mp_duvenaud_update_bwd_a_host, athena_mp_duvenaud_update_bwd_w_host
  public :: athena_mp_gno_aggregate_fwd_host, athena_mp_gno_aggregate_bwd_x_host, athena_mp_gno_aggregate_bwd_theta_host
  public :: athena_mp_gno_aggregate_bwd_coords_host
  public :: athena_mp_gemm_dw_host, athena_mp_gemm_dx_host, athena_mp_softmax_fwd_host, athena_mp_softmax_bwd_host
  public :: athena_mp_activation_fwd_host, athena_mp_activation_bwd_host
  public :: athena_mp_duvenaud_update_act_fwd_host, athena_mp_duvenaud_update_readout_fwd_host
  public :: athena_mp_duvenaud_update_bwd_pair_host, athena_mp_gno_aggregate_bwd_pair_host, athena_mp_pair_stats
  public :: athena_mp_malloc, athena_mp_free, athena_mp_memcpy_h2d, athena_mp_memcpy_d2h
  public :: athena_mp_kipf_propagate_fwd, athena_mp_kipf_propagate_bwd
  public :: athena_mp_gemm_fwd, athena_mp_gemm_dw, athena_mp_gemm_dx
  public :: athena_mp_adam_step, athena_mp_sgd_step, athena_mp_clip, athena_mp_mse_loss
  public :: athena_mp_swish_fwd, athena_mp_swish_bwd, athena_mp_softmax_fwd, athena_mp_softmax_bwd
  public :: athena_mp_concat_fwd, athena_mp_concat_bwd
  public :: athena_mp_activation_param_fwd, athena_mp_activation_param_bwd
  public :: athena_mp_memset_zero, athena_mp_activation_fwd, athena_mp_axpy, athena_mp_kipf_propagate_bwd_dual
  public :: athena_mp_kipf_propagate_act_fwd
  public :: athena_mp_reverse_kipf_propagate_fwd, athena_mp_reverse_kipf_propagate_partial
  public :: athena_mp_reverse_kipf_propagate_partial_val
  public :: athena_mp_duvenaud_propagate_fwd, athena_mp_duvenaud_propagate_bwd_x, athena_mp_duvenaud_propagate_bwd_e
  public :: athena_mp_duvenaud_update_bwd_a, athena_mp_duvenaud_update_bwd_w, athena_mp_duvenaud_update_bwd
  public :: athena_mp_duvenaud_update_bwd_split
  public :: athena_mp_duvenaud_readout_update_bwd
  public :: athena_mp_duvenaud_update_readout_fwd_split
  public :: athena_mp_duvenaud_update_readout_fwd
  public :: athena_mp_segment_sum, athena_mp_segment_sum_bwd
  public :: athena_mp_gno_aggregate_fwd, athena_mp_gno_aggregate_bwd_x, athena_mp_gno_aggregate_bwd_theta
  public :: athena_mp_gno_aggregate_bwd_coords
  public :: athena_mp_gno_saved_bytes, athena_mp_gno_aggregate_fwd_save, athena_mp_gno_aggregate_bwd_theta_saved
  public :: athena_mp_duvenaud_readout_fwd, athena_mp_duvenaud_readout_bwd, athena_mp_duvenaud_update_act_fwd
  public :: athena_mp_kipf_layer_fwd, athena_mp_kipf_layer_bwd_x, athena_mp_activation_bwd
  public :: athena_mp_csr_from_edges, athena_mp_graph_export, athena_mp_graph_create_from_edges
  public :: athena_mp_graph_create_from_edges_dev, athena_mp_radius_pairs, athena_mp_radius_graph_host
  public :: athena_mp_radius_pairs_batched, athena_mp_radius_graph_batched_host
  public :: athena_mp_radius_pairs_bipartite, athena_mp_graph_create_bipartite_dev, athena_mp_radius_graph_bipartite_host
  public :: athena_mp_edge_grad_to_point_sets, athena_mp_edge_grad_to_point_sets_host, athena_mp_add_row_bias
  public :: athena_mp_knn_pairs_batched, athena_mp_knn_pairs, athena_mp_knn_graph_batched_host, athena_mp_knn_stats
  public :: athena_mp_knn_pairs_bipartite, athena_mp_knn_graph_bipartite_host
  public :: athena_mp_farthest_points, athena_mp_farthest_points_host, athena_mp_fps_stats
  public :: athena_mp_grid_clusters, athena_mp_grid_clusters_grad, athena_mp_grid_clusters_host, athena_mp_grid_clusters_grad_host
  public :: athena_mp_grid_clusters_stats
  public :: athena_mp_contract_pairs, athena_mp_contract_pairs_host, athena_mp_contract_stats, athena_mp_graph_pairs
  public :: athena_mp_cell_pairs
  public :: athena_mp_topk_vertices, athena_mp_topk_vertices_host, athena_mp_topk_stats
  public :: athena_mp_select_rows_fwd, athena_mp_select_rows_bwd, athena_mp_select_rows_host, athena_mp_select_rows_bwd_host
  public :: athena_mp_interp_weights, athena_mp_interp_fwd, athena_mp_interp_bwd_x, athena_mp_interp_bwd_coords
  public :: athena_mp_interp_host, athena_mp_interp_bwd_host
  public :: athena_mp_pool_max_fwd, athena_mp_pool_max_edges_fwd, athena_mp_pool_max_bwd_x, athena_mp_pool_max_bwd_edges
  public :: athena_mp_pool_max_host, athena_mp_pool_max_bwd_host
  public :: athena_mp_attn_softmax_fwd, athena_mp_attn_gather_fwd, athena_mp_attn_gather_edges_fwd, athena_mp_attn_gather_bwd_x
  public :: athena_mp_attn_gather_bwd_edges, athena_mp_attn_gather_bwd_alpha, athena_mp_attn_softmax_bwd
  public :: athena_mp_attention_host, athena_mp_attention_bwd_host
  public :: athena_mp_triplet_pairs, athena_mp_entry_vectors_fwd, athena_mp_entry_vectors_bwd, athena_mp_triplet_cos_fwd
  public :: athena_mp_triplet_cos_bwd, athena_mp_triplet_stats, athena_mp_triplets_host, athena_mp_triplet_cos_bwd_host
  public :: athena_mp_edge_gather_fwd, athena_mp_edge_gather_bwd, athena_mp_edge_gather_host, athena_mp_edge_gather_bwd_host
  public :: athena_mp_periodic_pairs, athena_mp_periodic_graph_host, athena_mp_periodic_stats
  public :: athena_mp_edge_grad_to_points, athena_mp_periodic_grad
  public :: athena_mp_edge_grad_to_points_host, athena_mp_periodic_grad_host
  public :: athena_mp_batch_plan_create, athena_mp_batch_plan_destroy, athena_mp_batch_select
  public :: athena_mp_duvenaud_plan, athena_mp_duvenaud_plan_export, athena_mp_duvenaud_plan_stats
  public :: athena_mp_sampler_create, athena_mp_sampler_destroy, athena_mp_sample_count, athena_mp_sample_neighbors
  public :: athena_mp_sample_neighbors_host, athena_mp_sample_stats
  public :: athena_mp_error_message
  public :: athena_mp_pull_gemm, athena_mp_dev_offset, athena_mp_kipf_layer_bwd
  public :: athena_mp_comm_create, athena_mp_comm_create_from_file, athena_mp_comm_destroy, athena_mp_comm_barrier
  public :: athena_mp_comm_unique_id, athena_mp_allreduce, athena_mp_allreduce_start, athena_mp_allreduce_finish
  public :: athena_mp_shard_create, athena_mp_shard_destroy, athena_mp_shard_dims, athena_mp_shard_graph
  public :: athena_mp_shard_export, athena_mp_halo_start, athena_mp_halo_finish, athena_mp_shard_info
  public :: athena_mp_device_copy, athena_mp_gno_aggregate_bwd, athena_mp_halo_reduce_start, athena_mp_halo_reduce_finish
  public :: athena_mp_shard_edge_reduce
  public :: athena_mp_shard_create_edges, athena_mp_shard_edge_cols, athena_mp_gno_aggregate_bwd_x_pull
  public :: athena_mp_resident_mode, athena_mp_resident_acquire, athena_mp_resident_release, athena_mp_resident_flush
  public :: athena_mp_resident_drop, athena_mp_resident_stats

  interface
     integer(c_int) function athena_mp_init(device) bind(C, name="athena_mp_init")
       import :: c_int
       integer(c_int), value :: device
     end function
     integer(c_int) function athena_mp_initialized() bind(C, name="athena_mp_initialized")
       import :: c_int
     end function
     integer(c_int) function athena_mp_finalize() bind(C, name="athena_mp_finalize")
       import :: c_int
     end function
     integer(c_int) function athena_mp_synchronize() bind(C, name="athena_mp_synchronize")
       import :: c_int
     end function
     type(c_ptr) function athena_mp_last_error() bind(C, name="athena_mp_last_error")
       import :: c_ptr
     end function

     !! residency of host arrays (phase 2 for the *_host entry points): results stay in HBM until flushed at the edge of
     !! the HIP island (athena_network_sub.f90:2752,2761,2856); host_ptr = c_loc(array_type%val)
     integer(c_int) function athena_mp_resident_mode(on) bind(C, name="athena_mp_resident_mode")
       import :: c_int, c_int32_t
       integer(c_int32_t), value :: on
     end function
     integer(c_int) function athena_mp_resident_acquire(host_ptr, bytes, dirty_host, dev_ptr) &
          bind(C, name="athena_mp_resident_acquire")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value :: host_ptr
       integer(c_int64_t), value :: bytes
       integer(c_int32_t), value :: dirty_host
       type(c_ptr), intent(out) :: dev_ptr
     end function
     integer(c_int) function athena_mp_resident_release(host_ptr, dirty_dev) bind(C, name="athena_mp_resident_release")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: host_ptr
       integer(c_int32_t), value :: dirty_dev
     end function
     integer(c_int) function athena_mp_resident_flush(host_ptr) bind(C, name="athena_mp_resident_flush")
       import :: c_int, c_ptr
       type(c_ptr), value :: host_ptr              !! c_null_ptr: every array
     end function
     integer(c_int) function athena_mp_resident_drop(host_ptr) bind(C, name="athena_mp_resident_drop")
       import :: c_int, c_ptr
       type(c_ptr), value :: host_ptr
     end function
     integer(c_int) function athena_mp_resident_stats(arrays, h2d_bytes, d2h_bytes, reused_inputs, lazy_outputs) &
          bind(C, name="athena_mp_resident_stats")
       import :: c_int, c_int64_t
       integer(c_int64_t), intent(out) :: arrays, h2d_bytes, d2h_bytes, reused_inputs, lazy_outputs
     end function

     !! athena_msgpass_layer_sub.f90:144-174 (set_graph) -- build once, keep the handle
     integer(c_int) function athena_mp_graph_create(n_rows, n_cols, nnz, adj_ia, adj_ja, &
          n_edge_cols, row_deg, col_deg, graph) bind(C, name="athena_mp_graph_create")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int32_t), value :: n_rows, n_cols, n_edge_cols
       integer(c_int64_t), value :: nnz
       integer(c_int32_t), intent(in) :: adj_ia(*), adj_ja(2,*)
       type(c_ptr), value :: row_deg, col_deg        !! c_null_ptr: degrees = CSR row lengths
       type(c_ptr), intent(out) :: graph
     end function
     integer(c_int) function athena_mp_graph_destroy(graph) bind(C, name="athena_mp_graph_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: graph
     end function
     !! content key of (adj_ia, adj_ja): what a cached handle is valid for (SURVEY.md 8b "Ownership");
     !! key is C's uint64_t -- compared for equality only, so its bit pattern in an int64 serves
     pure integer(c_int) function athena_mp_graph_key(n_rows, nnz, adj_ia, adj_ja, key) &
          bind(C, name="athena_mp_graph_key")
       import :: c_int, c_int32_t, c_int64_t
       integer(c_int32_t), value :: n_rows
       integer(c_int64_t), value :: nnz
       integer(c_int32_t), intent(in) :: adj_ia(*), adj_ja(2,*)
       integer(c_int64_t), intent(out) :: key
     end function
     !! set_graph as a cache lookup (athena_network_sub.f90:2727-2730 calls set_graph before every forward):
     !! the shared, reference-counted handle of this CSR; built only when no live or idle handle matches
     integer(c_int) function athena_mp_graph_acquire(n, nnz, adj_ia, adj_ja, n_edge_cols, graph) &
          bind(C, name="athena_mp_graph_acquire")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int32_t), value :: n, n_edge_cols
       integer(c_int64_t), value :: nnz
       integer(c_int32_t), intent(in) :: adj_ia(*), adj_ja(2,*)
       type(c_ptr), intent(out) :: graph
     end function
     integer(c_int) function athena_mp_graph_release(graph) bind(C, name="athena_mp_graph_release")
       import :: c_int, c_ptr
       type(c_ptr), value :: graph
     end function
     !! release + the cache forgets the handle: after an in-place edit the caller announces (invalidate_graph)
     integer(c_int) function athena_mp_graph_evict(graph) bind(C, name="athena_mp_graph_evict")
       import :: c_int, c_ptr
       type(c_ptr), value :: graph
     end function
     integer(c_int) function athena_mp_graph_cache_stats(handles, hits, builds) &
          bind(C, name="athena_mp_graph_cache_stats")
       import :: c_int, c_int64_t
       integer(c_int64_t), intent(out) :: handles, hits, builds
     end function

     !! kipf_propagate, athena_diffstruc_extd_sub_kipf.f90:7-59 (host arrays, staged)
     pure integer(c_int) function athena_mp_kipf_propagate_fwd_host(graph, F, x, y) &
          bind(C, name="athena_mp_kipf_propagate_fwd_host")
       import :: c_int, c_int32_t, c_ptr, c_float
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: F
       real(c_float), intent(in) :: x(*)
       real(c_float), intent(inout) :: y(*)
     end function
     !! get_partial_kipf_propagate_left_val, ..._sub_kipf.f90:85-111
     pure integer(c_int) function athena_mp_kipf_propagate_bwd_host(graph, F, grad, dx, exact) &
          bind(C, name="athena_mp_kipf_propagate_bwd_host")
       import :: c_int, c_int32_t, c_ptr, c_float
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: F, exact
       real(c_float), intent(in) :: grad(*)
       real(c_float), intent(inout) :: dx(*)
     end function
     !! matmul(params(t), ptr2), athena_kipf_msgpass_layer.f90:951
     pure integer(c_int) function athena_mp_gemm_fwd_host(N, Fi, Fo, P, W, bias, act, Z) &
          bind(C, name="athena_mp_gemm_fwd_host")
       import :: c_int, c_int32_t, c_int64_t, c_ptr, c_float
       integer(c_int64_t), value :: N
       integer(c_int32_t), value :: Fi, Fo, act
       real(c_float), intent(in) :: P(*), W(*)
       type(c_ptr), value :: bias
       real(c_float), intent(inout) :: Z(*)
     end function

     !! duvenaud_propagate, athena_diffstruc_extd_sub_duvenaud.f90:7-59
     pure integer(c_int) function athena_mp_duvenaud_propagate_fwd_host(graph, Fv, Fe, x, e, c) &
          bind(C, name="athena_mp_duvenaud_propagate_fwd_host")
       import :: c_int, c_int32_t, c_ptr, c_float
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: Fv, Fe
       real(c_float), intent(in) :: x(*), e(*)
       real(c_float), intent(inout) :: c(*)
     end function
     !! get_partial_duvenaud_propagate_left_val, :115-141
     pure integer(c_int) function athena_mp_duvenaud_propagate_bwd_x_host(graph, Fv, Fe, grad, dx) &
          bind(C, name="athena_mp_duvenaud_propagate_bwd_x_host")
       import :: c_int, c_int32_t, c_ptr, c_float
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: Fv, Fe
       real(c_float), intent(in) :: grad(*)
       real(c_float), intent(inout) :: dx(*)
     end function
     !! duvenaud_update, :176-228
     pure integer(c_int) function athena_mp_duvenaud_update_fwd_host(graph, Fi, Fo, min_deg, max_deg, a, w, c) &
          bind(C, name="athena_mp_duvenaud_update_fwd_host")
       import :: c_int, c_int32_t, c_ptr, c_float
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: Fi, Fo, min_deg, max_deg
       real(c_float), intent(in) :: a(*), w(*)
       real(c_float), intent(inout) :: c(*)
     end function

     !! get_partial_duvenaud_propagate_right_val, :143-171
     pure integer(c_int) function athena_mp_duvenaud_propagate_bwd_e_host(graph, Fv, Fe, grad, de) &
          bind(C, name="athena_mp_duvenaud_propagate_bwd_e_host")
       import :: c_int, c_int32_t, c_ptr, c_float
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: Fv, Fe
       real(c_float), intent(in) :: grad(*)
       real(c_float), intent(inout) :: de(*)
     end function
     !! get_partial_duvenaud_update_val, :284-324
     pure integer(c_int) function athena_mp_duvenaud_update_bwd_a_host(graph, Fi, Fo, min_deg, max_deg, grad, w, da) &
          bind(C, name="athena_mp_duvenaud_update_bwd_a_host")
       import :: c_int, c_int32_t, c_ptr, c_float
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: Fi, Fo, min_deg, max_deg
       real(c_float), intent(in) :: grad(*), w(*)
       real(c_float), intent(inout) :: da(*)
     end function
     !! get_partial_duvenaud_update_weight_val, :326-368
     pure integer(c_int) function athena_mp_duvenaud_update_bwd_w_host(graph, Fi, Fo, min_deg, max_deg, grad, a, dw) &
          bind(C, name="athena_mp_duvenaud_update_bwd_w_host")
       import :: c_int, c_int32_t, c_ptr, c_float
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: Fi, Fo, min_deg, max_deg
       real(c_float), intent(in) :: grad(*), a(*)
       real(c_float), intent(inout) :: dw(*)
     end function
     !! gno_kernel_eval + gno_aggregate in one op (athena_diffstruc_extd_sub_nop.f90:26-115, :330-397): the per-edge kernel
     !! tensor is never formed; theta = U | b_u | V | b_v as gno_kernel_eval packs it (:74-82)
     pure integer(c_int) function athena_mp_gno_aggregate_fwd_host(graph, d, H, Fi, Fo, theta, coords, x, m) &
          bind(C, name="athena_mp_gno_aggregate_fwd_host")
       import :: c_int, c_int32_t, c_ptr, c_float
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: d, H, Fi, Fo
       real(c_float), intent(in) :: theta(*), coords(*), x(*)
       real(c_float), intent(inout) :: m(*)
     end function
     !! get_partial_gno_aggregate_features_val, :419-458 (through the kernels)
     pure integer(c_int) function athena_mp_gno_aggregate_bwd_x_host(graph, d, H, Fi, Fo, theta, coords, grad, dx) &
          bind(C, name="athena_mp_gno_aggregate_bwd_x_host")
       import :: c_int, c_int32_t, c_ptr, c_float
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: d, H, Fi, Fo
       real(c_float), intent(in) :: theta(*), coords(*), grad(*)
       real(c_float), intent(inout) :: dx(*)
     end function
     !! agg -> kernels (:480-526) chained with kernel -> params (:235-325)
     pure integer(c_int) function athena_mp_gno_aggregate_bwd_theta_host(graph, d, H, Fi, Fo, theta, coords, x, grad, dtheta) &
          bind(C, name="athena_mp_gno_aggregate_bwd_theta_host")
       import :: c_int, c_int32_t, c_ptr, c_float
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: d, H, Fi, Fo
       real(c_float), intent(in) :: theta(*), coords(*), x(*), grad(*)
       real(c_float), intent(inout) :: dtheta(*)
     end function
     !! agg -> kernels chained with kernel -> coords (:137-216)
     pure integer(c_int) function athena_mp_gno_aggregate_bwd_coords_host(graph, d, H, Fi, Fo, theta, coords, x, grad, &
          dcoords) bind(C, name="athena_mp_gno_aggregate_bwd_coords_host")
       import :: c_int, c_int32_t, c_ptr, c_float
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: d, H, Fi, Fo
       real(c_float), intent(in) :: theta(*), coords(*), x(*), grad(*)
       real(c_float), intent(inout) :: dcoords(*)
     end function

     !! ---- what a shim inside athena binds beyond the op-granular entry points (scripts/integration_check/) -----------
     !! the reverse of matmul, for composite nodes that own a dense step: dW = P^T dZ, dP = dZ W^T
     pure integer(c_int) function athena_mp_gemm_dw_host(N, Fi, Fo, P, dZ, dW) bind(C, name="athena_mp_gemm_dw_host")
       import :: c_int, c_int32_t, c_int64_t, c_float
       integer(c_int64_t), value :: N
       integer(c_int32_t), value :: Fi, Fo
       real(c_float), intent(in) :: P(*), dZ(*)
       real(c_float), intent(inout) :: dW(*)
     end function
     pure integer(c_int) function athena_mp_gemm_dx_host(N, Fi, Fo, dZ, W, dP) bind(C, name="athena_mp_gemm_dx_host")
       import :: c_int, c_int32_t, c_int64_t, c_float
       integer(c_int64_t), value :: N
       integer(c_int32_t), value :: Fi, Fo
       real(c_float), intent(in) :: dZ(*), W(*)
       real(c_float), intent(inout) :: dP(*)
     end function
     !! softmax over the features of every column (athena_diffstruc_extd_sub.f90:295-379) and its reverse at the OUTPUT
     pure integer(c_int) function athena_mp_softmax_fwd_host(N, F, z, y) bind(C, name="athena_mp_softmax_fwd_host")
       import :: c_int, c_int32_t, c_int64_t, c_float
       integer(c_int64_t), value :: N
       integer(c_int32_t), value :: F
       real(c_float), intent(in) :: z(*)
       real(c_float), intent(inout) :: y(*)
     end function
     pure integer(c_int) function athena_mp_softmax_bwd_host(N, F, y, g, dz) bind(C, name="athena_mp_softmax_bwd_host")
       import :: c_int, c_int32_t, c_int64_t, c_float
       integer(c_int64_t), value :: N
       integer(c_int32_t), value :: F
       real(c_float), intent(in) :: y(*), g(*)
       real(c_float), intent(inout) :: dz(*)
     end function
     pure integer(c_int) function athena_mp_activation_fwd_host(act, n, z, y) bind(C, name="athena_mp_activation_fwd_host")
       import :: c_int, c_int32_t, c_int64_t, c_float
       integer(c_int32_t), value :: act
       integer(c_int64_t), value :: n
       real(c_float), intent(in) :: z(*)
       real(c_float), intent(inout) :: y(*)
     end function
     pure integer(c_int) function athena_mp_activation_bwd_host(act, n, y, g, dz) bind(C, name="athena_mp_activation_bwd_host")
       import :: c_int, c_int32_t, c_int64_t, c_float
       integer(c_int32_t), value :: act
       integer(c_int64_t), value :: n
       real(c_float), intent(in) :: y(*), g(*)
       real(c_float), intent(inout) :: dz(*)
     end function
     !! update + message activation (+ the readout's per-vertex softmax(R z)) of one Duvenaud time step in ONE launch
     !! (athena_duvenaud_msgpass_layer.f90:790-803, 838-855)
     pure integer(c_int) function athena_mp_duvenaud_update_act_fwd_host(graph, Fi, Fo, min_deg, max_deg, a, w, act, z) &
          bind(C, name="athena_mp_duvenaud_update_act_fwd_host")
       import :: c_int, c_int32_t, c_ptr, c_float
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: Fi, Fo, min_deg, max_deg, act
       real(c_float), intent(in) :: a(*), w(*)
       real(c_float), intent(inout) :: z(*)
     end function
     pure integer(c_int) function athena_mp_duvenaud_update_readout_fwd_host(graph, Fi, Fo, min_deg, max_deg, a, w, act, z, &
          O, R, p) bind(C, name="athena_mp_duvenaud_update_readout_fwd_host")
       import :: c_int, c_int32_t, c_ptr, c_float
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: Fi, Fo, min_deg, max_deg, act, O
       real(c_float), intent(in) :: a(*), w(*), R(*)
       real(c_float), intent(inout) :: z(*), p(*)
     end function
     !! BOTH partials of a two-operand node from one device pass, across diffstruc's two stateless `pure` callbacks: the first
     !! request computes both and parks the other on the device, the second -- same handle, shapes and operand CONTENT -- takes
     !! it (include/athena_mp.h).  which: 0 = left operand's partial, 1 = right operand's (GNO: 2 = coordinates).
     !! act /= ATHENA_MP_ACT_NONE: the node is update + message activation in one; z = its value, grad the gradient w.r.t. z
     pure integer(c_int) function athena_mp_duvenaud_update_bwd_pair_host(graph, Fi, Fo, min_deg, max_deg, act, z, grad, a, w, &
          which, out) bind(C, name="athena_mp_duvenaud_update_bwd_pair_host")
       import :: c_int, c_int32_t, c_ptr, c_float
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: Fi, Fo, min_deg, max_deg, act, which
       real(c_float), intent(in) :: z(*), grad(*), a(*), w(*)
       real(c_float), intent(inout) :: out(*)
     end function
     pure integer(c_int) function athena_mp_gno_aggregate_bwd_pair_host(graph, d, H, Fi, Fo, theta, coords, x, grad, which, &
          out) bind(C, name="athena_mp_gno_aggregate_bwd_pair_host")
       import :: c_int, c_int32_t, c_ptr, c_float
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: d, H, Fi, Fo, which
       real(c_float), intent(in) :: theta(*), coords(*), x(*), grad(*)
       real(c_float), intent(inout) :: out(*)
     end function
     integer(c_int) function athena_mp_pair_stats(fused_passes, handed_over) bind(C, name="athena_mp_pair_stats")
       import :: c_int, c_int64_t
       integer(c_int64_t), intent(out) :: fused_passes, handed_over
     end function

     !! device-resident variants (phase 2: tensors stay in HBM between consecutive HIP layers)
     integer(c_int) function athena_mp_malloc(dev_ptr, bytes) bind(C, name="athena_mp_malloc")
       import :: c_int, c_ptr, c_int64_t
       type(c_ptr), intent(out) :: dev_ptr
       integer(c_int64_t), value :: bytes
     end function
     integer(c_int) function athena_mp_free(dev_ptr) bind(C, name="athena_mp_free")
       import :: c_int, c_ptr
       type(c_ptr), value :: dev_ptr
     end function
     integer(c_int) function athena_mp_memcpy_h2d(dst, src, bytes) bind(C, name="athena_mp_memcpy_h2d")
       import :: c_int, c_ptr, c_int64_t
       type(c_ptr), value :: dst
       type(*), dimension(*), intent(in) :: src        ! any host array (real32 tensors, int32 index arrays)
       integer(c_int64_t), value :: bytes
     end function
     integer(c_int) function athena_mp_memcpy_d2h(dst, src, bytes) bind(C, name="athena_mp_memcpy_d2h")
       import :: c_int, c_ptr, c_int64_t
       type(*), dimension(*), intent(inout) :: dst
       type(c_ptr), value :: src
       integer(c_int64_t), value :: bytes
     end function
     integer(c_int) function athena_mp_kipf_propagate_fwd(graph, F, x_dev, y_dev) &
          bind(C, name="athena_mp_kipf_propagate_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, x_dev, y_dev
       integer(c_int32_t), value :: F
     end function
     integer(c_int) function athena_mp_kipf_propagate_bwd(graph, F, g_dev, dx_dev, exact) &
          bind(C, name="athena_mp_kipf_propagate_bwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, g_dev, dx_dev
       integer(c_int32_t), value :: F, exact
     end function
     !! reverse_kipf_propagate and its partials, athena_diffstruc_extd_sub_kipf.f90:116-205
     integer(c_int) function athena_mp_reverse_kipf_propagate_fwd(graph, F, a_dev, c_dev) &
          bind(C, name="athena_mp_reverse_kipf_propagate_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, a_dev, c_dev
       integer(c_int32_t), value :: F
     end function
     integer(c_int) function athena_mp_reverse_kipf_propagate_partial(graph, F, up_dev, out_dev) &
          bind(C, name="athena_mp_reverse_kipf_propagate_partial")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, up_dev, out_dev
       integer(c_int32_t), value :: F
     end function
     integer(c_int) function athena_mp_reverse_kipf_propagate_partial_val(graph, F, up_dev, out_dev) &
          bind(C, name="athena_mp_reverse_kipf_propagate_partial_val")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, up_dev, out_dev
       integer(c_int32_t), value :: F
     end function
     integer(c_int) function athena_mp_gemm_fwd(N, Fi, Fo, P_dev, W_dev, bias_dev, act, Z_dev) &
          bind(C, name="athena_mp_gemm_fwd")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int64_t), value :: N
       integer(c_int32_t), value :: Fi, Fo, act
       type(c_ptr), value :: P_dev, W_dev, bias_dev, Z_dev
     end function
     integer(c_int) function athena_mp_gemm_dw(N, Fi, Fo, P_dev, dZ_dev, dW_dev) &
          bind(C, name="athena_mp_gemm_dw")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int64_t), value :: N
       integer(c_int32_t), value :: Fi, Fo
       type(c_ptr), value :: P_dev, dZ_dev, dW_dev
     end function
     integer(c_int) function athena_mp_gemm_dx(N, Fi, Fo, dZ_dev, W_dev, dP_dev) &
          bind(C, name="athena_mp_gemm_dx")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int64_t), value :: N
       integer(c_int32_t), value :: Fi, Fo
       type(c_ptr), value :: dZ_dev, W_dev, dP_dev
     end function

     !! edge list -> CSR on the device (graphstruc's generate_adjacency [+ add_self_loops]); adj_ja = c_null_ptr queries nnz
     integer(c_int) function athena_mp_csr_from_edges(n_vertices, n_pairs, index_list, add_self_loops, adj_ia, &
          adj_ja, capacity, nnz) bind(C, name="athena_mp_csr_from_edges")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int32_t), value :: n_vertices, add_self_loops
       integer(c_int64_t), value :: n_pairs, capacity
       integer(c_int32_t), intent(in) :: index_list(2,*)
       integer(c_int32_t), intent(inout) :: adj_ia(*)
       type(c_ptr), value :: adj_ja                     !! c_loc of an integer(c_int32_t) adj_ja(2,capacity) target
       integer(c_int64_t), intent(out) :: nnz
     end function
     !! edge list -> CSR -> handle with the entries staying in HBM in between; adj_ja_out = c_null_ptr: not wanted
     integer(c_int) function athena_mp_graph_create_from_edges(n_vertices, n_pairs, index_list, add_self_loops, &
          with_edge_ids, adj_ia, adj_ja, capacity, nnz, graph) bind(C, name="athena_mp_graph_create_from_edges")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int32_t), value :: n_vertices, add_self_loops, with_edge_ids
       integer(c_int64_t), value :: n_pairs, capacity
       integer(c_int32_t), intent(in) :: index_list(2,*)
       integer(c_int32_t), intent(inout) :: adj_ia(*)
       type(c_ptr), value :: adj_ja
       integer(c_int64_t), intent(out) :: nnz
       type(c_ptr), intent(out) :: graph
     end function
     !! the same for an index list that is already in HBM (index_list_dev: the pair list athena_mp_radius_pairs wrote)
     integer(c_int) function athena_mp_graph_create_from_edges_dev(n_vertices, n_pairs, index_list_dev, add_self_loops, &
          with_edge_ids, adj_ia, adj_ja, capacity, nnz, graph) bind(C, name="athena_mp_graph_create_from_edges_dev")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int32_t), value :: n_vertices, add_self_loops, with_edge_ids
       integer(c_int64_t), value :: n_pairs, capacity
       type(c_ptr), value :: index_list_dev
       integer(c_int32_t), intent(inout) :: adj_ia(*)
       type(c_ptr), value :: adj_ja
       integer(c_int64_t), intent(out) :: nnz
       type(c_ptr), intent(out) :: graph
     end function
     !! points (dim, n) on the device -> pair list (2, capacity) and coords (dim, capacity) on the device, pairs in
     !! lexicographic order of (i, j), i < j; both outputs c_null_ptr: n_pairs only (definition: include/athena_mp.h)
     integer(c_int) function athena_mp_radius_pairs(n, dim, points_dev, radius, pairs_dev, coords_dev, capacity, n_pairs) &
          bind(C, name="athena_mp_radius_pairs")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n, dim
       type(c_ptr), value :: points_dev, pairs_dev, coords_dev
       real(c_float), value :: radius
       integer(c_int64_t), value :: capacity
       integer(c_int64_t), intent(out) :: n_pairs
     end function
     !! the same with host arrays: points (dim, n) -> adj_ia (n + 1), adj_ja (2, capacity), coords (dim, coords_capacity);
     !! adj_ja = c_null_ptr queries nnz and n_pairs (adj_ia and coords may then be c_null_ptr too)
     integer(c_int) function athena_mp_radius_graph_host(n, dim, points, radius, add_self_loops, adj_ia, adj_ja, capacity, &
          nnz, coords, coords_capacity, n_pairs) bind(C, name="athena_mp_radius_graph_host")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n, dim, add_self_loops
       real(c_float), intent(in) :: points(dim, *)
       real(c_float), value :: radius
       type(c_ptr), value :: adj_ia, adj_ja, coords     !! c_loc of adj_ia(n+1), adj_ja(2,capacity), coords(dim,coords_capacity)
       integer(c_int64_t), value :: capacity, coords_capacity
       integer(c_int64_t), intent(out) :: nnz, n_pairs
     end function
     !! a batch of point clouds -> ONE block-diagonal pair list: offsets (n_clouds + 1) on the host, 0-based, ascending from 0 to n;
     !! points (dim, n) on the device -> pairs (2, capacity) and coords (dim, capacity) on the device, each may be c_null_ptr (both:
     !! n_pairs and edge_offsets only).  edge_offsets: c_loc of an integer(c_int64_t) (n_clouds + 1) host array, or c_null_ptr
     !! (definition: include/athena_mp.h)
     integer(c_int) function athena_mp_radius_pairs_batched(n_clouds, n, offsets, dim, points_dev, radius, pairs_dev, coords_dev, &
          capacity, edge_offsets, n_pairs) bind(C, name="athena_mp_radius_pairs_batched")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n_clouds, n, dim
       integer(c_int32_t), intent(in) :: offsets(*)
       type(c_ptr), value :: points_dev, pairs_dev, coords_dev, edge_offsets
       real(c_float), value :: radius
       integer(c_int64_t), value :: capacity
       integer(c_int64_t), intent(out) :: n_pairs
     end function
     !! the same with host arrays: points (dim, n) -> adj_ia (n + 1), adj_ja (2, capacity), coords (dim, coords_capacity),
     !! edge_offsets (n_clouds + 1); adj_ja = c_null_ptr queries nnz, n_pairs and edge_offsets
     integer(c_int) function athena_mp_radius_graph_batched_host(n_clouds, n, offsets, dim, points, radius, add_self_loops, &
          adj_ia, adj_ja, capacity, nnz, coords, coords_capacity, n_pairs, edge_offsets) &
          bind(C, name="athena_mp_radius_graph_batched_host")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n_clouds, n, dim, add_self_loops
       integer(c_int32_t), intent(in) :: offsets(*)
       real(c_float), intent(in) :: points(dim, *)
       real(c_float), value :: radius
       type(c_ptr), value :: adj_ia, adj_ja, coords, edge_offsets
       integer(c_int64_t), value :: capacity, coords_capacity
       integer(c_int64_t), intent(out) :: nnz, n_pairs
     end function
     !! radius graphs between TWO point sets, a batch of clouds per call (definition: include/athena_mp.h): query_offsets and
     !! source_offsets (n_clouds + 1) on the host, 0-based; queries (dim, n_queries) and sources (dim, n_sources) on the device ->
     !! pairs (2, capacity) = (query, source), coords (dim, capacity) = query minus source and rowptr (n_queries + 1, 0-based) on
     !! the device, each may be c_null_ptr (all three: n_pairs and edge_offsets only).  edge_offsets: c_loc of an
     !! integer(c_int64_t) (n_clouds + 1) host array, or c_null_ptr
     integer(c_int) function athena_mp_radius_pairs_bipartite(n_clouds, n_queries, query_offsets, n_sources, source_offsets, dim, &
          queries_dev, sources_dev, radius, pairs_dev, coords_dev, capacity, rowptr_dev, edge_offsets, n_pairs) &
          bind(C, name="athena_mp_radius_pairs_bipartite")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n_clouds, n_queries, n_sources, dim
       integer(c_int32_t), intent(in) :: query_offsets(*), source_offsets(*)
       type(c_ptr), value :: queries_dev, sources_dev, pairs_dev, coords_dev, rowptr_dev, edge_offsets
       real(c_float), value :: radius
       integer(c_int64_t), value :: capacity
       integer(c_int64_t), intent(out) :: n_pairs
     end function
     !! such a pair list in HBM -> the directed rectangular handle (pair e = the one entry (row i, column j, edge id e)); adj_ia
     !! (n_rows + 1) is always filled, adj_ja: c_loc of (2, capacity) on the host, or c_null_ptr
     integer(c_int) function athena_mp_graph_create_bipartite_dev(n_rows, n_cols, n_pairs, pairs_dev, adj_ia, adj_ja, capacity, &
          graph) bind(C, name="athena_mp_graph_create_bipartite_dev")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int32_t), value :: n_rows, n_cols
       integer(c_int64_t), value :: n_pairs, capacity
       type(c_ptr), value :: pairs_dev, adj_ja
       integer(c_int32_t), intent(inout) :: adj_ia(*)
       type(c_ptr), intent(out) :: graph
     end function
     !! the search with host arrays: queries (dim, n_queries), sources (dim, n_sources) -> adj_ia (n_queries + 1), adj_ja
     !! (2, capacity) = (source, edge id), coords (dim, coords_capacity), edge_offsets (n_clouds + 1); adj_ja = c_null_ptr queries
     !! n_pairs and edge_offsets
     integer(c_int) function athena_mp_radius_graph_bipartite_host(n_clouds, n_queries, query_offsets, n_sources, source_offsets, &
          dim, queries, sources, radius, adj_ia, adj_ja, capacity, coords, coords_capacity, edge_offsets, n_pairs) &
          bind(C, name="athena_mp_radius_graph_bipartite_host")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n_clouds, n_queries, n_sources, dim
       integer(c_int32_t), intent(in) :: query_offsets(*), source_offsets(*)
       real(c_float), intent(in) :: queries(dim, *), sources(dim, *)
       real(c_float), value :: radius
       type(c_ptr), value :: adj_ia, adj_ja, coords, edge_offsets
       integer(c_int64_t), value :: capacity, coords_capacity
       integer(c_int64_t), intent(out) :: n_pairs
     end function
     !! a batch of point clouds -> ONE block-diagonal k-nearest-neighbour pair list (definition: include/athena_mp.h): the first k
     !! others of every point in the order (squared distance, index), inside radius when it is finite (ieee +infinity: no cap);
     !! mode 0 = union, 1 = mutual.  nbr (k, n), pairs (2, capacity), coords (dim, capacity) on the device, each may be
     !! c_null_ptr (all three: n_pairs and edge_offsets only); capacity = n * k always suffices
     integer(c_int) function athena_mp_knn_pairs_batched(n_clouds, n, offsets, dim, points_dev, k, radius, mode, nbr_dev, pairs_dev, &
          coords_dev, capacity, edge_offsets, n_pairs) bind(C, name="athena_mp_knn_pairs_batched")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n_clouds, n, dim, k, mode
       integer(c_int32_t), intent(in) :: offsets(*)
       type(c_ptr), value :: points_dev, nbr_dev, pairs_dev, coords_dev, edge_offsets
       real(c_float), value :: radius
       integer(c_int64_t), value :: capacity
       integer(c_int64_t), intent(out) :: n_pairs
     end function
     !! the same for one cloud
     integer(c_int) function athena_mp_knn_pairs(n, dim, points_dev, k, radius, mode, nbr_dev, pairs_dev, coords_dev, capacity, &
          n_pairs) bind(C, name="athena_mp_knn_pairs")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n, dim, k, mode
       type(c_ptr), value :: points_dev, nbr_dev, pairs_dev, coords_dev
       real(c_float), value :: radius
       integer(c_int64_t), value :: capacity
       integer(c_int64_t), intent(out) :: n_pairs
     end function
     !! the same with host arrays: points (dim, n) -> adj_ia (n + 1), adj_ja (2, capacity), coords (dim, coords_capacity),
     !! edge_offsets (n_clouds + 1); adj_ja = c_null_ptr queries nnz, n_pairs and edge_offsets
     integer(c_int) function athena_mp_knn_graph_batched_host(n_clouds, n, offsets, dim, points, k, radius, mode, add_self_loops, &
          adj_ia, adj_ja, capacity, nnz, coords, coords_capacity, n_pairs, edge_offsets) &
          bind(C, name="athena_mp_knn_graph_batched_host")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n_clouds, n, dim, k, mode, add_self_loops
       integer(c_int32_t), intent(in) :: offsets(*)
       real(c_float), intent(in) :: points(dim, *)
       real(c_float), value :: radius
       type(c_ptr), value :: adj_ia, adj_ja, coords, edge_offsets
       integer(c_int64_t), value :: capacity, coords_capacity
       integer(c_int64_t), intent(out) :: nnz, n_pairs
     end function
     !! the search of the last k-nearest-neighbour call: queries, candidates examined, cells visited, the largest shell
     integer(c_int) function athena_mp_knn_stats(out) bind(C, name="athena_mp_knn_stats")
       import :: c_int, c_int64_t
       integer(c_int64_t), intent(out) :: out(4)
     end function
     !! k-nearest-neighbour graphs between TWO point sets, a batch of clouds per call (definition: include/athena_mp.h): every
     !! query joined to the first k sources of its cloud in the order (squared distance, index), inside radius when it is finite
     !! (ieee +infinity: no cap).  Inputs as athena_mp_radius_pairs_bipartite; nbr (k, n_queries) and sqdist (k, n_queries) in key
     !! order, pairs (2, capacity) = (query, source), coords (dim, capacity) and rowptr (n_queries + 1, 0-based) on the device,
     !! each may be c_null_ptr (all five: n_pairs and edge_offsets only); capacity = n_queries * k always suffices
     integer(c_int) function athena_mp_knn_pairs_bipartite(n_clouds, n_queries, query_offsets, n_sources, source_offsets, dim, &
          queries_dev, sources_dev, k, radius, nbr_dev, sqdist_dev, pairs_dev, coords_dev, capacity, rowptr_dev, edge_offsets, &
          n_pairs) bind(C, name="athena_mp_knn_pairs_bipartite")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n_clouds, n_queries, n_sources, dim, k
       integer(c_int32_t), intent(in) :: query_offsets(*), source_offsets(*)
       type(c_ptr), value :: queries_dev, sources_dev, nbr_dev, sqdist_dev, pairs_dev, coords_dev, rowptr_dev, edge_offsets
       real(c_float), value :: radius
       integer(c_int64_t), value :: capacity
       integer(c_int64_t), intent(out) :: n_pairs
     end function
     !! the same with host arrays: queries (dim, n_queries), sources (dim, n_sources) -> adj_ia (n_queries + 1), adj_ja
     !! (2, capacity) = (source, edge id), coords (dim, coords_capacity), nbr and sqdist (k, n_queries; c_null_ptr: not wanted),
     !! edge_offsets (n_clouds + 1); adj_ja = c_null_ptr queries n_pairs and edge_offsets
     integer(c_int) function athena_mp_knn_graph_bipartite_host(n_clouds, n_queries, query_offsets, n_sources, source_offsets, dim, &
          queries, sources, k, radius, adj_ia, adj_ja, capacity, coords, coords_capacity, nbr, sqdist, edge_offsets, n_pairs) &
          bind(C, name="athena_mp_knn_graph_bipartite_host")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n_clouds, n_queries, n_sources, dim, k
       integer(c_int32_t), intent(in) :: query_offsets(*), source_offsets(*)
       real(c_float), intent(in) :: queries(dim, *), sources(dim, *)
       real(c_float), value :: radius
       type(c_ptr), value :: adj_ia, adj_ja, coords, nbr, sqdist, edge_offsets
       integer(c_int64_t), value :: capacity, coords_capacity
       integer(c_int64_t), intent(out) :: n_pairs
     end function
     !! farthest-point sampling of a batch of clouds (definition: include/athena_mp.h): cloud b gets sample_offsets(b+1) -
     !! sample_offsets(b) of its own points, the first one start(b) (1-based global; 0: the cloud's first point), each next one
     !! the point not yet chosen that is farthest from those chosen, ties to the smaller index.  offsets, sample_offsets
     !! (n_clouds + 1) and start (c_loc of n_clouds int32, or c_null_ptr) on the host; points (dim, n) on the device; sample
     !! (n_samples), sample_points (dim, n_samples), sample_sqdist (n_samples) and cover_sqdist (n_clouds) on the device, each
     !! may be c_null_ptr
     integer(c_int) function athena_mp_farthest_points(n_clouds, n, offsets, dim, points_dev, n_samples, sample_offsets, start, &
          sample_dev, sample_points_dev, sample_sqdist_dev, cover_sqdist_dev) bind(C, name="athena_mp_farthest_points")
       import :: c_int, c_int32_t, c_ptr
       integer(c_int32_t), value :: n_clouds, n, dim, n_samples
       integer(c_int32_t), intent(in) :: offsets(*), sample_offsets(*)
       type(c_ptr), value :: points_dev, start, sample_dev, sample_points_dev, sample_sqdist_dev, cover_sqdist_dev
     end function
     !! the same with host arrays: points (dim, n) -> sample, sample_points, sample_sqdist, cover_sqdist (c_null_ptr: not wanted)
     integer(c_int) function athena_mp_farthest_points_host(n_clouds, n, offsets, dim, points, n_samples, sample_offsets, start, &
          sample, sample_points, sample_sqdist, cover_sqdist) bind(C, name="athena_mp_farthest_points_host")
       import :: c_int, c_int32_t, c_float, c_ptr
       integer(c_int32_t), value :: n_clouds, n, dim, n_samples
       integer(c_int32_t), intent(in) :: offsets(*), sample_offsets(*)
       real(c_float), intent(in) :: points(dim, *)
       type(c_ptr), value :: start, sample, sample_points, sample_sqdist, cover_sqdist
     end function
     !! the last farthest-point call: samples, chunk tests of the stream route, tests that skipped, clouds on the stream route
     integer(c_int) function athena_mp_fps_stats(out) bind(C, name="athena_mp_fps_stats")
       import :: c_int, c_int64_t
       integer(c_int64_t), intent(out) :: out(4)
     end function
     !! voxel-grid clusters of a batch of clouds (definition: include/athena_mp.h): every non-empty cubic cell of edge size of a
     !! cloud is one cluster, numbered by (cloud, cell) with the first axis fastest, members in index order.  offsets
     !! (n_clouds + 1) and origin (c_loc of dim real32, or c_null_ptr: each cloud's own lower corner) on the host; points (dim, n)
     !! on the device; cluster (n), pairs (2, n) = (cluster, point), rowptr (capacity + 1, 0-based), weights (n), centroid
     !! (dim, capacity), nearest (capacity) and cell (dim, capacity) on the device, each may be c_null_ptr (all seven: the counts
     !! only); cluster_offsets (c_loc of n_clouds + 1 int32) and origin_out (c_loc of (dim, n_clouds) real32) on the host, or
     !! c_null_ptr
     integer(c_int) function athena_mp_grid_clusters(n_clouds, n, offsets, dim, points_dev, size, origin, capacity, cluster_dev, &
          pairs_dev, rowptr_dev, weights_dev, centroid_dev, nearest_dev, cell_dev, cluster_offsets, origin_out, n_clusters) &
          bind(C, name="athena_mp_grid_clusters")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n_clouds, n, dim
       integer(c_int32_t), intent(in) :: offsets(*)
       real(c_float), value :: size
       integer(c_int64_t), value :: capacity
       type(c_ptr), value :: points_dev, origin, cluster_dev, pairs_dev, rowptr_dev, weights_dev, centroid_dev, nearest_dev, cell_dev
       type(c_ptr), value :: cluster_offsets, origin_out
       integer(c_int64_t), intent(out) :: n_clusters
     end function
     !! its reverse step: dpoints(:, j) = dcentroid(:, cluster(j)) / count of that cluster, count from the differences of rowptr
     integer(c_int) function athena_mp_grid_clusters_grad(n, dim, n_clusters, cluster_dev, rowptr_dev, dcentroid_dev, dpoints_dev) &
          bind(C, name="athena_mp_grid_clusters_grad")
       import :: c_int, c_int32_t, c_ptr
       integer(c_int32_t), value :: n, dim, n_clusters
       type(c_ptr), value :: cluster_dev, rowptr_dev, dcentroid_dev, dpoints_dev
     end function
     !! the same with host arrays: points (dim, n) -> adj_ia (capacity + 1, 1-based), adj_ja (2, n) = (point, edge id), and
     !! cluster (n), weights (n), centroid (dim, capacity), nearest (capacity), cell (dim, capacity), cluster_offsets
     !! (n_clouds + 1), origin_out (dim, n_clouds) (c_null_ptr: not wanted); adj_ja = c_null_ptr queries n_clusters,
     !! cluster_offsets and origin_out
     integer(c_int) function athena_mp_grid_clusters_host(n_clouds, n, offsets, dim, points, size, origin, capacity, cluster, adj_ia, &
          adj_ja, weights, centroid, nearest, cell, cluster_offsets, origin_out, n_clusters) &
          bind(C, name="athena_mp_grid_clusters_host")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n_clouds, n, dim
       integer(c_int32_t), intent(in) :: offsets(*)
       real(c_float), intent(in) :: points(dim, *)
       real(c_float), value :: size
       integer(c_int64_t), value :: capacity
       type(c_ptr), value :: origin, cluster, adj_ia, adj_ja, weights, centroid, nearest, cell, cluster_offsets, origin_out
       integer(c_int64_t), intent(out) :: n_clusters
     end function
     !! ... and its reverse step: cluster (n), rowptr (n_clusters + 1: adj_ia serves), dcentroid (dim, n_clusters) -> dpoints (dim, n)
     integer(c_int) function athena_mp_grid_clusters_grad_host(n, dim, n_clusters, cluster, rowptr, dcentroid, dpoints) &
          bind(C, name="athena_mp_grid_clusters_grad_host")
       import :: c_int, c_int32_t, c_float
       integer(c_int32_t), value :: n, dim, n_clusters
       integer(c_int32_t), intent(in) :: cluster(*), rowptr(*)
       real(c_float), intent(in) :: dcentroid(dim, *)
       real(c_float), intent(out) :: dpoints(dim, *)
     end function
     !! the last grid-cluster call: clusters, key bits sorted, radix passes, members of the largest cluster
     integer(c_int) function athena_mp_grid_clusters_stats(out) bind(C, name="athena_mp_grid_clusters_stats")
       import :: c_int, c_int64_t
       integer(c_int64_t), intent(out) :: out(4)
     end function
     !! a pair list relabelled through a vertex map and merged (definition: include/athena_mp.h): graph contraction over a cluster
     !! map, the induced subgraph of a selection (id 0 drops a vertex), the merge of duplicate pairs (no maps).  Everything on the
     !! device: pairs (2, n_pairs), row_cluster (n_rows), col_cluster (n_cols) (c_null_ptr: the identity), row_points
     !! (dim, m_rows), col_points (dim, m_cols) (both or neither); outputs coarse_pairs (2, capacity), rowptr (capacity + 1,
     !! 0-based), members (2, member_capacity) = (coarse pair, fine edge), weights (member_capacity), edge_pair (n_pairs), coords
     !! (dim, capacity), each may be c_null_ptr (all six: the counts only).  mode 0: undirected, one set; 1: directed, two sets
     integer(c_int) function athena_mp_contract_pairs(n_pairs, pairs_dev, n_rows, n_cols, row_cluster_dev, col_cluster_dev, m_rows, &
          m_cols, mode, dim, row_points_dev, col_points_dev, capacity, member_capacity, coarse_pairs_dev, rowptr_dev, members_dev, &
          weights_dev, edge_pair_dev, coords_dev, n_coarse, n_members) bind(C, name="athena_mp_contract_pairs")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int64_t), value :: n_pairs, capacity, member_capacity
       integer(c_int32_t), value :: n_rows, n_cols, m_rows, m_cols, mode, dim
       type(c_ptr), value :: pairs_dev, row_cluster_dev, col_cluster_dev, row_points_dev, col_points_dev
       type(c_ptr), value :: coarse_pairs_dev, rowptr_dev, members_dev, weights_dev, edge_pair_dev, coords_dev
       integer(c_int64_t), intent(out) :: n_coarse, n_members
     end function
     !! the same with host arrays, staged through HBM: pairs (2, n_pairs); the maps, the points and the six outputs as c_loc of
     !! host arrays of the shapes above, or c_null_ptr
     integer(c_int) function athena_mp_contract_pairs_host(n_pairs, pairs, n_rows, n_cols, row_cluster, col_cluster, m_rows, m_cols, &
          mode, dim, row_points, col_points, capacity, member_capacity, coarse_pairs, rowptr, members, weights, edge_pair, coords, &
          n_coarse, n_members) bind(C, name="athena_mp_contract_pairs_host")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int64_t), value :: n_pairs, capacity, member_capacity
       integer(c_int32_t), intent(in) :: pairs(2, *)
       integer(c_int32_t), value :: n_rows, n_cols, m_rows, m_cols, mode, dim
       type(c_ptr), value :: row_cluster, col_cluster, row_points, col_points
       type(c_ptr), value :: coarse_pairs, rowptr, members, weights, edge_pair, coords
       integer(c_int64_t), intent(out) :: n_coarse, n_members
     end function
     !! the last contraction call: coarse pairs, members, key bits sorted, members of the largest coarse pair
     integer(c_int) function athena_mp_contract_stats(out) bind(C, name="athena_mp_contract_stats")
       import :: c_int, c_int64_t
       integer(c_int64_t), intent(out) :: out(4)
     end function
     !! a handle's pair list on the device: pairs (2, n_edge_cols), (row, column) of the first entry that carries each edge column
     integer(c_int) function athena_mp_graph_pairs(graph, pairs_dev, capacity) bind(C, name="athena_mp_graph_pairs")
       import :: c_int, c_int64_t, c_ptr
       type(c_ptr), value :: graph, pairs_dev
       integer(c_int64_t), value :: capacity
     end function
     !! mesh elements -> pair list on the device: cells (nv, n_cells) 1-based; cell_type 1 segment, 2 triangle, 3 quadrilateral
     !! (its ring), 4 tetrahedron; pairs (2, capacity), slot (c - 1) * ne + l = local pair l of cell c; pairs_dev = c_null_ptr: the
     !! count and the check only
     integer(c_int) function athena_mp_cell_pairs(n_vertices, n_cells, cell_type, cells_dev, pairs_dev, capacity, n_pairs) &
          bind(C, name="athena_mp_cell_pairs")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int32_t), value :: n_vertices, cell_type
       integer(c_int64_t), value :: n_cells, capacity
       type(c_ptr), value :: cells_dev, pairs_dev
       integer(c_int64_t), intent(out) :: n_pairs
     end function
     !! top-k vertex selection per graph from scores on the device (definition: include/athena_mp.h): offsets (n_graphs + 1) on
     !! the host, 0-based; score (n) on the device; k_each (n_graphs) on the host or c_null_ptr and then k for every graph ->
     !! cluster (n), selected (m), order (m) on the device, sel_offsets (n_graphs + 1) on the host (c_null_ptr: not wanted);
     !! selected and order hold the sum of min(k_g, n_g) elements
     integer(c_int) function athena_mp_topk_vertices(n_graphs, n, offsets, score_dev, k, k_each, has_min_score, min_score, &
          cluster_dev, selected_dev, order_dev, sel_offsets, n_selected) bind(C, name="athena_mp_topk_vertices")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n_graphs, n, k, has_min_score
       integer(c_int32_t), intent(in) :: offsets(*)
       real(c_float), value :: min_score
       type(c_ptr), value :: score_dev, k_each, cluster_dev, selected_dev, order_dev, sel_offsets
       integer(c_int64_t), intent(out) :: n_selected
     end function
     !! the same with host arrays
     integer(c_int) function athena_mp_topk_vertices_host(n_graphs, n, offsets, score, k, k_each, has_min_score, min_score, &
          cluster, selected, order, sel_offsets, n_selected) bind(C, name="athena_mp_topk_vertices_host")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n_graphs, n, k, has_min_score
       integer(c_int32_t), intent(in) :: offsets(*)
       real(c_float), intent(in) :: score(*)
       real(c_float), value :: min_score
       type(c_ptr), value :: k_each, cluster, selected, order, sel_offsets
       integer(c_int64_t), intent(out) :: n_selected
     end function
     !! the last selection call: graphs on the wave route, graphs on the sort route, key bits sorted, radix passes
     integer(c_int) function athena_mp_topk_stats(out) bind(C, name="athena_mp_topk_stats")
       import :: c_int, c_int64_t
       integer(c_int64_t), intent(out) :: out(4)
     end function
     !! the rows of a selection, gated: x (F, n), gate (n) or c_null_ptr, selected (m) -> y (F, m) = x(:, selected) * gate
     integer(c_int) function athena_mp_select_rows_fwd(n, m, F, selected_dev, x_dev, gate_dev, y_dev) &
          bind(C, name="athena_mp_select_rows_fwd")
       import :: c_int, c_int32_t, c_ptr
       integer(c_int32_t), value :: n, m, F
       type(c_ptr), value :: selected_dev, x_dev, gate_dev, y_dev
     end function
     !! ... and the reverse: cluster (n), dy (F, m) -> dx (F, n), dgate (n) (either may be c_null_ptr; dgate needs x)
     integer(c_int) function athena_mp_select_rows_bwd(n, m, F, cluster_dev, dy_dev, x_dev, gate_dev, dx_dev, dgate_dev) &
          bind(C, name="athena_mp_select_rows_bwd")
       import :: c_int, c_int32_t, c_ptr
       integer(c_int32_t), value :: n, m, F
       type(c_ptr), value :: cluster_dev, dy_dev, x_dev, gate_dev, dx_dev, dgate_dev
     end function
     !! the two with host arrays
     integer(c_int) function athena_mp_select_rows_host(n, m, F, selected, x, gate, y) bind(C, name="athena_mp_select_rows_host")
       import :: c_int, c_int32_t, c_float, c_ptr
       integer(c_int32_t), value :: n, m, F
       integer(c_int32_t), intent(in) :: selected(*)
       real(c_float), intent(in) :: x(F, *)
       type(c_ptr), value :: gate
       real(c_float), intent(out) :: y(F, *)
     end function
     integer(c_int) function athena_mp_select_rows_bwd_host(n, m, F, cluster, dy, x, gate, dx, dgate) &
          bind(C, name="athena_mp_select_rows_bwd_host")
       import :: c_int, c_int32_t, c_float, c_ptr
       integer(c_int32_t), value :: n, m, F
       integer(c_int32_t), intent(in) :: cluster(*)
       real(c_float), intent(in) :: dy(F, *)
       type(c_ptr), value :: x, gate, dx, dgate
     end function
     !! periodic structures -> pair list and edge geometry on the device, a batch per call (replaces get_graph_from_basis;
     !! definition: include/athena_mp.h).  offsets (n_structures + 1) and pbc (3) on the host; frac (3, n_atoms) and
     !! lat (3, 3, n_structures) -- lat(c, a, s) = component c of lattice vector a, i.e. transpose(basis%lat) -- on the device;
     !! outputs on the device: pairs (2, capacity), feature (capacity), vec (3, capacity), shift (3, capacity),
     !! first_count (n_atoms), each may be c_null_ptr; all five c_null_ptr: n_pairs only.  edge_offsets: c_loc of an
     !! integer(c_int64_t) (n_structures + 1) host array, or c_null_ptr
     integer(c_int) function athena_mp_periodic_pairs(n_structures, n_atoms, offsets, frac_dev, lat_dev, pbc, cutoff_min, &
          cutoff_max, pairs_dev, feature_dev, vec_dev, shift_dev, first_count_dev, capacity, n_pairs, edge_offsets) &
          bind(C, name="athena_mp_periodic_pairs")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n_structures, n_atoms
       integer(c_int32_t), intent(in) :: offsets(*), pbc(3)
       type(c_ptr), value :: frac_dev, lat_dev, pairs_dev, feature_dev, vec_dev, shift_dev, first_count_dev, edge_offsets
       real(c_float), value :: cutoff_min, cutoff_max
       integer(c_int64_t), value :: capacity
       integer(c_int64_t), intent(out) :: n_pairs
     end function
     !! the same with host arrays: -> adj_ia (n_atoms + 1), adj_ja (2, capacity), feature (edge_capacity),
     !! vec (3, edge_capacity), first_count (n_atoms), edge_offsets (n_structures + 1, int64), all passed as c_loc;
     !! adj_ja = c_null_ptr queries nnz and n_pairs (the other outputs may then be c_null_ptr too)
     integer(c_int) function athena_mp_periodic_graph_host(n_structures, n_atoms, offsets, frac, lat, pbc, cutoff_min, &
          cutoff_max, add_self_loops, adj_ia, adj_ja, capacity, nnz, feature, vec, first_count, edge_capacity, n_pairs, &
          edge_offsets) bind(C, name="athena_mp_periodic_graph_host")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: n_structures, n_atoms, add_self_loops
       integer(c_int32_t), intent(in) :: offsets(*), pbc(3)
       real(c_float), intent(in) :: frac(3, *), lat(3, 3, *)
       real(c_float), value :: cutoff_min, cutoff_max
       type(c_ptr), value :: adj_ia, adj_ja, feature, vec, first_count, edge_offsets
       integer(c_int64_t), value :: capacity, edge_capacity
       integer(c_int64_t), intent(out) :: nnz, n_pairs
     end function
     !! what the most recent periodic build did: structures walked, structures through the cell grid, pairs of the walk,
     !! candidate pairs of the grid, structures that qualified for the grid but took the walk
     integer(c_int) function athena_mp_periodic_stats(stats) bind(C, name="athena_mp_periodic_stats")
       import :: c_int, c_int64_t
       integer(c_int64_t), intent(out) :: stats(5)
     end function
     !! geometry gradients, the reverse step of the two builders (definition: include/athena_mp.h).  The reverse of
     !! athena_mp_radius_pairs: dcoords (dim, E) on the device -> dpoints (dim, n) on the device, a signed sum over the handle's rows
     integer(c_int) function athena_mp_edge_grad_to_points(graph, dim, dcoords_dev, dpoints_dev) &
          bind(C, name="athena_mp_edge_grad_to_points")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, dcoords_dev, dpoints_dev
       integer(c_int32_t), value :: dim
     end function
     !! the reverse of athena_mp_periodic_pairs: offsets and edge_offsets (n_structures + 1) on the host; lat (3, 3, n_structures),
     !! vec (3, E), dfeature (fe_cols, E), dvec (3, E) on the device (one of the last two may be c_null_ptr) -> dcart (3, n_atoms),
     !! dfrac (3, n_atoms), virial (3, 3, n_structures), dlat (3, 3, n_structures) on the device, each may be c_null_ptr.
     !! virial(d, c, s) = sum x_c gx_d and dlat(d, a, s) = dE/dL[a][d]: the row-major [B, 3, 3] arrays of the C side
     integer(c_int) function athena_mp_periodic_grad(graph, n_structures, n_atoms, offsets, edge_offsets, lat_dev, cutoff_max, &
          vec_dev, dfeature_dev, fe_cols, dvec_dev, dcart_dev, dfrac_dev, virial_dev, dlat_dev) &
          bind(C, name="athena_mp_periodic_grad")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       type(c_ptr), value :: graph, lat_dev, vec_dev, dfeature_dev, dvec_dev, dcart_dev, dfrac_dev, virial_dev, dlat_dev
       integer(c_int32_t), value :: n_structures, n_atoms, fe_cols
       integer(c_int32_t), intent(in) :: offsets(*)
       integer(c_int64_t), intent(in) :: edge_offsets(*)
       real(c_float), value :: cutoff_max
     end function
     !! the same two with host arrays (staged): dcoords (dim, E) -> dpoints (dim, n)
     integer(c_int) function athena_mp_edge_grad_to_points_host(graph, dim, dcoords, dpoints) &
          bind(C, name="athena_mp_edge_grad_to_points_host")
       import :: c_int, c_int32_t, c_float, c_ptr
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: dim
       real(c_float), intent(in) :: dcoords(dim, *)
       real(c_float), intent(inout) :: dpoints(dim, *)
     end function
     !! the reverse of athena_mp_radius_pairs_bipartite on its rectangular handle: dcoords (dim, E) -> dqueries (dim, n_rows) = the
     !! sum over each row, dsources (dim, n_cols) = minus the sum over each column; each output may be c_null_ptr, not both
     integer(c_int) function athena_mp_edge_grad_to_point_sets(graph, dim, dcoords_dev, dqueries_dev, dsources_dev) &
          bind(C, name="athena_mp_edge_grad_to_point_sets")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, dcoords_dev, dqueries_dev, dsources_dev
       integer(c_int32_t), value :: dim
     end function
     !! the same with host arrays (staged); dqueries, dsources: c_loc of the host arrays, or c_null_ptr
     integer(c_int) function athena_mp_edge_grad_to_point_sets_host(graph, dim, dcoords, dqueries, dsources) &
          bind(C, name="athena_mp_edge_grad_to_point_sets_host")
       import :: c_int, c_int32_t, c_float, c_ptr
       type(c_ptr), value :: graph, dqueries, dsources
       integer(c_int32_t), value :: dim
       real(c_float), intent(in) :: dcoords(dim, *)
     end function
     !! inverse-distance interpolation over a two-set handle (definition: include/athena_mp.h): the weights of coords (dim, E) ->
     !! weights (E), wsum (n_rows) or c_null_ptr
     integer(c_int) function athena_mp_interp_weights(graph, dim, coords_dev, eps, weights_dev, wsum_dev) &
          bind(C, name="athena_mp_interp_weights")
       import :: c_int, c_int32_t, c_float, c_ptr
       type(c_ptr), value :: graph, coords_dev, weights_dev, wsum_dev
       integer(c_int32_t), value :: dim
       real(c_float), value :: eps
     end function
     !! the weighted gather over the rows, x (F, n_cols) -> y (F, n_rows), for any weights (E) ...
     integer(c_int) function athena_mp_interp_fwd(graph, F, weights_dev, x_dev, y_dev) bind(C, name="athena_mp_interp_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, weights_dev, x_dev, y_dev
       integer(c_int32_t), value :: F
     end function
     !! ... and over the columns, dy (F, n_rows) -> dx (F, n_cols)
     integer(c_int) function athena_mp_interp_bwd_x(graph, F, weights_dev, dy_dev, dx_dev) bind(C, name="athena_mp_interp_bwd_x")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, weights_dev, dy_dev, dx_dev
       integer(c_int32_t), value :: F
     end function
     !! the gradient with respect to coords through the weights: dcoords (dim, E), what athena_mp_edge_grad_to_point_sets takes
     integer(c_int) function athena_mp_interp_bwd_coords(graph, dim, F, coords_dev, eps, weights_dev, x_dev, y_dev, dy_dev, &
          dcoords_dev) bind(C, name="athena_mp_interp_bwd_coords")
       import :: c_int, c_int32_t, c_float, c_ptr
       type(c_ptr), value :: graph, coords_dev, weights_dev, x_dev, y_dev, dy_dev, dcoords_dev
       integer(c_int32_t), value :: dim, F
       real(c_float), value :: eps
     end function
     !! the same with host arrays (staged): coords (dim, E), x (F, n_cols) -> y (F, n_rows); weights: c_loc of (E), or c_null_ptr
     integer(c_int) function athena_mp_interp_host(graph, dim, F, coords, eps, x, y, weights) bind(C, name="athena_mp_interp_host")
       import :: c_int, c_int32_t, c_float, c_ptr
       type(c_ptr), value :: graph, weights
       integer(c_int32_t), value :: dim, F
       real(c_float), value :: eps
       real(c_float), intent(in) :: coords(dim, *), x(F, *)
       real(c_float), intent(inout) :: y(F, *)
     end function
     !! ... and dy (F, n_rows) -> dx (F, n_cols), dcoords (dim, E): c_loc of the host arrays, or c_null_ptr (not both)
     integer(c_int) function athena_mp_interp_bwd_host(graph, dim, F, coords, eps, x, dy, dx, dcoords) &
          bind(C, name="athena_mp_interp_bwd_host")
       import :: c_int, c_int32_t, c_float, c_ptr
       type(c_ptr), value :: graph, dx, dcoords
       integer(c_int32_t), value :: dim, F
       real(c_float), value :: eps
       real(c_float), intent(in) :: coords(dim, *), x(F, *), dy(F, *)
     end function
     !! max pooling over a handle's rows with its arg-max (definition: include/athena_mp.h): x (F, n_cols) -> y (F, n_rows) and
     !! arg (F, n_rows) int32, the 0-based column of the first maximum, -1 along an empty row; arg_dev may be c_null_ptr
     integer(c_int) function athena_mp_pool_max_fwd(graph, F, x_dev, y_dev, arg_dev) bind(C, name="athena_mp_pool_max_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, x_dev, y_dev, arg_dev
       integer(c_int32_t), value :: F
     end function
     !! ... the same over per-edge values h (F, E), on a handle with one entry per edge column
     integer(c_int) function athena_mp_pool_max_edges_fwd(graph, F, h_dev, y_dev, arg_dev) &
          bind(C, name="athena_mp_pool_max_edges_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, h_dev, y_dev, arg_dev
       integer(c_int32_t), value :: F
     end function
     !! the reverse of the vertex form: dy (F, n_rows) -> dx (F, n_cols), each column's sum over the rows that chose it, ascending
     integer(c_int) function athena_mp_pool_max_bwd_x(graph, F, arg_dev, dy_dev, dx_dev) bind(C, name="athena_mp_pool_max_bwd_x")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, arg_dev, dy_dev, dx_dev
       integer(c_int32_t), value :: F
     end function
     !! the reverse of the edge form: dy (F, n_rows) -> dh (F, E), dy of the row where the edge was chosen, else 0
     integer(c_int) function athena_mp_pool_max_bwd_edges(graph, F, arg_dev, dy_dev, dh_dev) &
          bind(C, name="athena_mp_pool_max_bwd_edges")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, arg_dev, dy_dev, dh_dev
       integer(c_int32_t), value :: F
     end function
     !! the same with host arrays (staged): exactly one of x (F, n_cols) and h (F, E) is c_loc of the host array, the other
     !! c_null_ptr; arg: c_loc of (F, n_rows) int32, or c_null_ptr
     integer(c_int) function athena_mp_pool_max_host(graph, F, x, h, y, arg) bind(C, name="athena_mp_pool_max_host")
       import :: c_int, c_int32_t, c_float, c_ptr
       type(c_ptr), value :: graph, x, h, arg
       integer(c_int32_t), value :: F
       real(c_float), intent(inout) :: y(F, *)
     end function
     !! ... and arg, dy (F, n_rows) -> dx (F, n_cols), dh (F, E): c_loc of the host arrays, or c_null_ptr (not both)
     integer(c_int) function athena_mp_pool_max_bwd_host(graph, F, arg, dy, dx, dh) bind(C, name="athena_mp_pool_max_bwd_host")
       import :: c_int, c_int32_t, c_float, c_ptr
       type(c_ptr), value :: graph, dx, dh
       integer(c_int32_t), value :: F
       integer(c_int32_t), intent(in) :: arg(F, *)
       real(c_float), intent(in) :: dy(F, *)
     end function
     !! bond-angle triplets of a square handle with edge columns (definition: include/athena_mp.h): pairs_dev (2, capacity) int32, the
     !! 1-based entry pairs athena_mp_graph_create_bipartite_dev(nnz, nnz, T, ...) takes; rowptr_dev (nnz + 1) int32 or c_null_ptr; both
     !! c_null_ptr: size query.  vec_dev (dim, E) may be c_null_ptr with cutoff3 = +infinity
     integer(c_int) function athena_mp_triplet_pairs(graph, dim, vec_dev, cutoff3, pairs_dev, capacity, rowptr_dev, n_triplets) &
          bind(C, name="athena_mp_triplet_pairs")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       type(c_ptr), value :: graph, vec_dev, pairs_dev, rowptr_dev
       integer(c_int32_t), value :: dim
       real(c_float), value :: cutoff3
       integer(c_int64_t), value :: capacity
       integer(c_int64_t), intent(out) :: n_triplets
     end function
     !! vec (dim, E) -> dir (dim, nnz), the vector from each entry's row vertex to its neighbour, and back: ddir -> dvec
     integer(c_int) function athena_mp_entry_vectors_fwd(graph, dim, vec_dev, dir_dev) bind(C, name="athena_mp_entry_vectors_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, vec_dev, dir_dev
       integer(c_int32_t), value :: dim
     end function
     integer(c_int) function athena_mp_entry_vectors_bwd(graph, dim, ddir_dev, dvec_dev) bind(C, name="athena_mp_entry_vectors_bwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, ddir_dev, dvec_dev
       integer(c_int32_t), value :: dim
     end function
     !! on the triplet handle: dir (dim, nnz) -> cos (T), and dir, cos, dcos (T) -> ddir (dim, nnz)
     integer(c_int) function athena_mp_triplet_cos_fwd(tgraph, dim, dir_dev, cos_dev) bind(C, name="athena_mp_triplet_cos_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: tgraph, dir_dev, cos_dev
       integer(c_int32_t), value :: dim
     end function
     integer(c_int) function athena_mp_triplet_cos_bwd(tgraph, dim, dir_dev, cos_dev, dcos_dev, ddir_dev) &
          bind(C, name="athena_mp_triplet_cos_bwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: tgraph, dir_dev, cos_dev, dcos_dev, ddir_dev
       integer(c_int32_t), value :: dim
     end function
     !! triplets, participants and the longest run of the last athena_mp_triplet_pairs
     integer(c_int) function athena_mp_triplet_stats(stats) bind(C, name="athena_mp_triplet_stats")
       import :: c_int, c_int64_t
       integer(c_int64_t), intent(out) :: stats(3)
     end function
     !! the same with host arrays: adj_ia (nnz + 1) 1-based, adj_ja (2, capacity) (second entry, triplet id), c_null_ptr for the size
     !! query; dir (dim, nnz) and cos (T): c_loc of the host arrays, or c_null_ptr; vec: c_loc of (dim, E), or c_null_ptr
     integer(c_int) function athena_mp_triplets_host(graph, dim, vec, cutoff3, adj_ia, adj_ja, capacity, dir, cosv, n_triplets) &
          bind(C, name="athena_mp_triplets_host")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       type(c_ptr), value :: graph, vec, adj_ia, adj_ja, dir, cosv
       integer(c_int32_t), value :: dim
       real(c_float), value :: cutoff3
       integer(c_int64_t), value :: capacity
       integer(c_int64_t), intent(out) :: n_triplets
     end function
     !! ... and dcos (n_triplets) -> dvec (dim, E) in one call; the triplet handle is built and freed inside
     integer(c_int) function athena_mp_triplet_cos_bwd_host(graph, dim, vec, cutoff3, n_triplets, dcos, dvec) &
          bind(C, name="athena_mp_triplet_cos_bwd_host")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: dim
       real(c_float), value :: cutoff3
       integer(c_int64_t), value :: n_triplets
       real(c_float), intent(in) :: vec(dim, *), dcos(*)
       real(c_float), intent(inout) :: dvec(dim, *)
     end function
     !! attention pooling over a handle's rows (definition: include/athena_mp.h), on a handle with one entry per edge column; H = n_heads,
     !! the head of feature c (0-based) is c / (F / H).  The softmax over each row's entries, per head: scores (H, E) -> alpha (H, E)
     integer(c_int) function athena_mp_attn_softmax_fwd(graph, n_heads, scores_dev, alpha_dev) bind(C, name="athena_mp_attn_softmax_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, scores_dev, alpha_dev
       integer(c_int32_t), value :: n_heads
     end function
     !! the weighted sum over each row, the weight chosen per head: alpha (H, E), x (F, n_cols) -> y (F, n_rows)
     integer(c_int) function athena_mp_attn_gather_fwd(graph, F, n_heads, alpha_dev, x_dev, y_dev) bind(C, name="athena_mp_attn_gather_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, alpha_dev, x_dev, y_dev
       integer(c_int32_t), value :: F, n_heads
     end function
     !! ... the same over per-edge values h (F, E)
     integer(c_int) function athena_mp_attn_gather_edges_fwd(graph, F, n_heads, alpha_dev, h_dev, y_dev) &
          bind(C, name="athena_mp_attn_gather_edges_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, alpha_dev, h_dev, y_dev
       integer(c_int32_t), value :: F, n_heads
     end function
     !! the reverse of the vertex form: dy (F, n_rows) -> dx (F, n_cols), each column's sum over its queries, ascending
     integer(c_int) function athena_mp_attn_gather_bwd_x(graph, F, n_heads, alpha_dev, dy_dev, dx_dev) &
          bind(C, name="athena_mp_attn_gather_bwd_x")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, alpha_dev, dy_dev, dx_dev
       integer(c_int32_t), value :: F, n_heads
     end function
     !! the reverse of the edge form: dy (F, n_rows) -> dh (F, E) = alpha * dy of the edge's row
     integer(c_int) function athena_mp_attn_gather_bwd_edges(graph, F, n_heads, alpha_dev, dy_dev, dh_dev) &
          bind(C, name="athena_mp_attn_gather_bwd_edges")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, alpha_dev, dy_dev, dh_dev
       integer(c_int32_t), value :: F, n_heads
     end function
     !! the reverse with respect to the weights: exactly one of x_dev (F, n_cols) and h_dev (F, E), the other c_null_ptr -> dalpha (H, E)
     integer(c_int) function athena_mp_attn_gather_bwd_alpha(graph, F, n_heads, x_dev, h_dev, dy_dev, dalpha_dev) &
          bind(C, name="athena_mp_attn_gather_bwd_alpha")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, x_dev, h_dev, dy_dev, dalpha_dev
       integer(c_int32_t), value :: F, n_heads
     end function
     !! the reverse of the softmax: alpha, dalpha (H, E) -> dscores (H, E)
     integer(c_int) function athena_mp_attn_softmax_bwd(graph, n_heads, alpha_dev, dalpha_dev, dscores_dev) &
          bind(C, name="athena_mp_attn_softmax_bwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, alpha_dev, dalpha_dev, dscores_dev
       integer(c_int32_t), value :: n_heads
     end function
     !! the same with host arrays (staged): scores (H, E) -> alpha (c_loc of (H, E), or c_null_ptr) and y (F, n_rows) over exactly one of
     !! x (F, n_cols) and h (F, E): c_loc of the host array, the other c_null_ptr
     integer(c_int) function athena_mp_attention_host(graph, F, n_heads, scores, x, h, alpha, y) bind(C, name="athena_mp_attention_host")
       import :: c_int, c_int32_t, c_float, c_ptr
       type(c_ptr), value :: graph, x, h, alpha
       integer(c_int32_t), value :: F, n_heads
       real(c_float), intent(in) :: scores(n_heads, *)
       real(c_float), intent(inout) :: y(F, *)
     end function
     !! ... and alpha (H, E), the same one of x and h, dy (F, n_rows) -> dx (F, n_cols) or dh (F, E), and dscores (H, E): c_loc of the
     !! host arrays, or c_null_ptr (not all three)
     integer(c_int) function athena_mp_attention_bwd_host(graph, F, n_heads, alpha, x, h, dy, dx, dh, dscores) &
          bind(C, name="athena_mp_attention_bwd_host")
       import :: c_int, c_int32_t, c_float, c_ptr
       type(c_ptr), value :: graph, x, h, dx, dh, dscores
       integer(c_int32_t), value :: F, n_heads
       real(c_float), intent(in) :: alpha(n_heads, *), dy(F, *)
     end function
     !! the edge MLP's input over a two-set handle (definition: include/athena_mp.h): h (ld, E), column e = xs(:, j) (relative = 1:
     !! less xq(:, i)), then xq(:, i), then coords(:, e) for the entry (i, j) of edge e; ld >= Fs + Fq + dim, the elements beyond
     !! stay as they are; a block of width 0 is c_null_ptr
     integer(c_int) function athena_mp_edge_gather_fwd(graph, Fs, xs_dev, Fq, xq_dev, dim, coords_dev, relative, ld, h_dev) &
          bind(C, name="athena_mp_edge_gather_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, xs_dev, xq_dev, coords_dev, h_dev
       integer(c_int32_t), value :: Fs, Fq, dim, relative, ld
     end function
     !! its reverse: dh (ld, E) -> dxs (Fs, n_cols), dxq (Fq, n_rows), dcoords (dim, E), each a device pointer or c_null_ptr
     integer(c_int) function athena_mp_edge_gather_bwd(graph, Fs, Fq, dim, relative, ld, dh_dev, dxs_dev, dxq_dev, dcoords_dev) &
          bind(C, name="athena_mp_edge_gather_bwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, dh_dev, dxs_dev, dxq_dev, dcoords_dev
       integer(c_int32_t), value :: Fs, Fq, dim, relative, ld
     end function
     !! the same with host arrays (staged): xs, xq, coords are c_loc of the host arrays, c_null_ptr for a block of width 0
     integer(c_int) function athena_mp_edge_gather_host(graph, Fs, xs, Fq, xq, dim, coords, relative, ld, h) &
          bind(C, name="athena_mp_edge_gather_host")
       import :: c_int, c_int32_t, c_float, c_ptr
       type(c_ptr), value :: graph, xs, xq, coords
       integer(c_int32_t), value :: Fs, Fq, dim, relative, ld
       real(c_float), intent(inout) :: h(ld, *)
     end function
     !! ... and dh (ld, E) -> dxs, dxq, dcoords: c_loc of the host arrays, or c_null_ptr (not all three)
     integer(c_int) function athena_mp_edge_gather_bwd_host(graph, Fs, Fq, dim, relative, ld, dh, dxs, dxq, dcoords) &
          bind(C, name="athena_mp_edge_gather_bwd_host")
       import :: c_int, c_int32_t, c_float, c_ptr
       type(c_ptr), value :: graph, dxs, dxq, dcoords
       integer(c_int32_t), value :: Fs, Fq, dim, relative, ld
       real(c_float), intent(in) :: dh(ld, *)
     end function
     !! ... dfeature, dvec and the four outputs passed as c_loc of host arrays, or c_null_ptr
     integer(c_int) function athena_mp_periodic_grad_host(graph, n_structures, n_atoms, offsets, edge_offsets, lat, cutoff_max, &
          vec, dfeature, fe_cols, dvec, dcart, dfrac, virial, dlat) bind(C, name="athena_mp_periodic_grad_host")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       type(c_ptr), value :: graph, dfeature, dvec, dcart, dfrac, virial, dlat
       integer(c_int32_t), value :: n_structures, n_atoms, fe_cols
       integer(c_int32_t), intent(in) :: offsets(*)
       integer(c_int64_t), intent(in) :: edge_offsets(*)
       real(c_float), intent(in) :: lat(3, 3, *), vec(3, *)
       real(c_float), value :: cutoff_max
     end function
     !! mini-batches out of a dataset handle that stays on the device (definition: include/athena_mp.h).  The plan: offsets and
     !! edge_offsets (n_structures + 1) on the host, 0-based; edge_offsets = c_null_ptr for a handle without edge columns
     integer(c_int) function athena_mp_batch_plan_create(graph, n_structures, offsets, edge_offsets, plan) &
          bind(C, name="athena_mp_batch_plan_create")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, edge_offsets
       integer(c_int32_t), value :: n_structures
       integer(c_int32_t), intent(in) :: offsets(*)
       type(c_ptr), intent(out) :: plan
     end function
     integer(c_int) function athena_mp_batch_plan_destroy(plan) bind(C, name="athena_mp_batch_plan_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan
     end function
     !! sel (n_sel) 0-based structure ids on the host -> the child handle; offsets_out (n_sel + 1, int32) and edge_offsets_out
     !! (n_sel + 1, int64) as c_loc of host arrays, vertex_map_dev / edge_map_dev device pointers: each may be c_null_ptr.
     !! child = c_loc of a type(c_ptr), target variable that receives the handle; child = c_null_ptr is the size query
     integer(c_int) function athena_mp_batch_select(plan, n_sel, sel, child, offsets_out, edge_offsets_out, vertex_map_dev, &
          edge_map_dev) bind(C, name="athena_mp_batch_select")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: plan, child, offsets_out, edge_offsets_out, vertex_map_dev, edge_map_dev
       integer(c_int32_t), value :: n_sel
       integer(c_int32_t), intent(in) :: sel(*)
     end function
     !! Neighbour-sampled mini-batches of ONE large graph (definition: include/athena_mp.h).  The sampler plan borrows the parent
     !! handle (n_rows == n_cols) and must be destroyed before it.  Every id is 1-based.
     integer(c_int) function athena_mp_sampler_create(parent, sampler) bind(C, name="athena_mp_sampler_create")
       import :: c_int, c_ptr
       type(c_ptr), value :: parent
       type(c_ptr), intent(out) :: sampler
     end function
     integer(c_int) function athena_mp_sampler_destroy(sampler) bind(C, name="athena_mp_sampler_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: sampler
     end function
     !! the count pass alone: seeds_dev (n_seeds) a device pointer, rowptr_dev (n_seeds + 1, 0-based) a device pointer or c_null_ptr
     integer(c_int) function athena_mp_sample_count(sampler, n_seeds, seeds_dev, k, rowptr_dev, nnz) bind(C, name="athena_mp_sample_count")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value :: sampler, seeds_dev, rowptr_dev
       integer(c_int32_t), value :: n_seeds, k
       integer(c_int64_t), intent(out) :: nnz
     end function
     !! one hop on device arrays: the three maps are device pointers with their capacities in elements, each may be c_null_ptr;
     !! block = c_loc of a type(c_ptr), target variable that receives the handle, or c_null_ptr.  degree_mode 0 = block, 1 = parent
     integer(c_int) function athena_mp_sample_neighbors(sampler, n_seeds, seeds_dev, k, seed, degree_mode, vertex_map_dev, &
          vertex_capacity, entry_map_dev, entry_capacity, edge_map_dev, edge_capacity, n_cols, nnz, block) &
          bind(C, name="athena_mp_sample_neighbors")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value :: sampler, seeds_dev, vertex_map_dev, entry_map_dev, edge_map_dev, block
       integer(c_int32_t), value :: n_seeds, k, degree_mode
       integer(c_int64_t), value :: seed, vertex_capacity, entry_capacity, edge_capacity
       integer(c_int32_t), intent(out) :: n_cols
       integer(c_int64_t), intent(out) :: nnz
     end function
     !! one hop on Fortran arrays: seeds (n_seeds); vertex_map (vertex_capacity), entry_map, edge_map (entry_capacity), adj_ia
     !! (n_seeds + 1) and adj_ja (2, entry_capacity) as c_loc of host arrays, the maps each may be c_null_ptr; adj_ja = c_null_ptr
     !! is the size query for n_cols and nnz.  seed: the 64 bits of the definition's unsigned seed
     integer(c_int) function athena_mp_sample_neighbors_host(sampler, n_seeds, seeds, k, seed, degree_mode, vertex_capacity, &
          entry_capacity, vertex_map, entry_map, edge_map, adj_ia, adj_ja, n_cols, nnz, block) &
          bind(C, name="athena_mp_sample_neighbors_host")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value :: sampler, vertex_map, entry_map, edge_map, adj_ia, adj_ja, block
       integer(c_int32_t), value :: n_seeds, k, degree_mode
       integer(c_int32_t), intent(in) :: seeds(*)
       integer(c_int64_t), value :: seed, vertex_capacity, entry_capacity
       integer(c_int32_t), intent(out) :: n_cols
       integer(c_int64_t), intent(out) :: nnz
     end function
     !! of the last sample: rows drawn, rows copied whole, steps, steps skipped, then four times in microseconds
     integer(c_int) function athena_mp_sample_stats(stats) bind(C, name="athena_mp_sample_stats")
       import :: c_int, c_int64_t
       integer(c_int64_t), intent(out) :: stats(8)
     end function
     !! the Duvenaud degree-bucket plan of a handle (definition: include/athena_mp.h): built now, on the library's stream; a no-op
     !! when the handle already holds the plan of (min_deg, max_deg).  Called right after athena_mp_batch_select on the child
     integer(c_int) function athena_mp_duvenaud_plan(graph, min_deg, max_deg) bind(C, name="athena_mp_duvenaud_plan")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: min_deg, max_deg
     end function
     !! one array of the plan back on the host (which 0..6: see include/athena_mp.h; 5 is int64); host_dst = c_null_ptr queries count
     integer(c_int) function athena_mp_duvenaud_plan_export(graph, which, host_dst, capacity, count) &
          bind(C, name="athena_mp_duvenaud_plan_export")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value :: graph, host_dst
       integer(c_int32_t), value :: which
       integer(c_int64_t), value :: capacity
       integer(c_int64_t), intent(out) :: count
     end function
     !! plans built on the host / on the device by this process, requests served by a plan the handle already held
     integer(c_int) function athena_mp_duvenaud_plan_stats(host_builds, device_builds, reused) &
          bind(C, name="athena_mp_duvenaud_plan_stats")
       import :: c_int, c_int64_t
       integer(c_int64_t), intent(out) :: host_builds, device_builds, reused
     end function
     !! one array of the handle back on the host (which: see include/athena_mp.h); host_dst = c_null_ptr queries count
     integer(c_int) function athena_mp_graph_export(graph, which, host_dst, capacity, count) &
          bind(C, name="athena_mp_graph_export")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value :: graph, host_dst
       integer(c_int32_t), value :: which
       integer(c_int64_t), value :: capacity
       integer(c_int64_t), intent(out) :: count
     end function

     !! ---- one-launch Kipf layer step on device-resident arrays (update_message_kipf :943-952 and its reverse) ----
     integer(c_int) function athena_mp_kipf_layer_fwd(graph, Fi, Fo, x_dev, W_dev, bias_dev, act, P_dev, Z_dev) &
          bind(C, name="athena_mp_kipf_layer_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, x_dev, W_dev, bias_dev, P_dev, Z_dev
       integer(c_int32_t), value :: Fi, Fo, act
     end function
     integer(c_int) function athena_mp_kipf_layer_bwd_x(graph, Fi, Fo, dZ_dev, W_dev, exact, dX_dev) &
          bind(C, name="athena_mp_kipf_layer_bwd_x")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, dZ_dev, W_dev, dX_dev
       integer(c_int32_t), value :: Fi, Fo, exact
     end function
     integer(c_int) function athena_mp_activation_bwd(act, n, y_dev, g_dev, dz_dev) &
          bind(C, name="athena_mp_activation_bwd")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int32_t), value :: act
       integer(c_int64_t), value :: n
       type(c_ptr), value :: y_dev, g_dev, dz_dev
     end function

     !! ---- device-resident tail of a train step (network%update, athena_network_sub.f90:2816-2929) ----
     !! minimise_adam, athena_optimiser.f90:1027-1091 (iter = optimiser%iter after the increment)
     integer(c_int) function athena_mp_adam_step(n, lr, beta1, beta2, epsilon, iter, reg_kind, l1, l2, &
          decoupled, param_dev, grad_dev, m_dev, v_dev) bind(C, name="athena_mp_adam_step")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int64_t), value :: n
       real(c_float), value :: lr, beta1, beta2, epsilon, l1, l2
       integer(c_int32_t), value :: iter, reg_kind, decoupled
       type(c_ptr), value :: param_dev, grad_dev, m_dev, v_dev
     end function
     !! minimise_sgd, athena_optimiser.f90:634-673
     integer(c_int) function athena_mp_sgd_step(n, lr, momentum, nesterov, reg_kind, l1, l2, &
          param_dev, grad_dev, velocity_dev) bind(C, name="athena_mp_sgd_step")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int64_t), value :: n
       real(c_float), value :: lr, momentum, l1, l2
       integer(c_int32_t), value :: nesterov, reg_kind
       type(c_ptr), value :: param_dev, grad_dev, velocity_dev
     end function
     !! apply_clip, athena_clipper.f90:165-210
     integer(c_int) function athena_mp_clip(n, grad_dev, l_min_max, clip_min, clip_max, l_norm, clip_norm) &
          bind(C, name="athena_mp_clip")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int64_t), value :: n
       type(c_ptr), value :: grad_dev
       integer(c_int32_t), value :: l_min_max, l_norm
       real(c_float), value :: clip_min, clip_max, clip_norm
     end function
     !! compute_mse, athena_loss.f90:393-430
     integer(c_int) function athena_mp_mse_loss(n, pred_dev, expected_dev, loss_dev, dpred_dev) &
          bind(C, name="athena_mp_mse_loss")
       import :: c_int, c_int64_t, c_ptr
       integer(c_int64_t), value :: n
       type(c_ptr), value :: pred_dev, expected_dev, loss_dev, dpred_dev
     end function

     !! ---- activations with attributes (kind: 0 linear, 1 relu(threshold), 2 sigmoid, 3 tanh,
     !!      4 leaky_relu(alpha), 5 selu(alpha, lambda), 6 gaussian(sigma, mu), 7 piecewise(gradient, limit)) ----
     integer(c_int) function athena_mp_activation_param_fwd(kind, n, scale, p0, p1, x_dev, y_dev) &
          bind(C, name="athena_mp_activation_param_fwd")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: kind
       integer(c_int64_t), value :: n
       real(c_float), value :: scale, p0, p1
       type(c_ptr), value :: x_dev, y_dev
     end function
     integer(c_int) function athena_mp_activation_param_bwd(kind, n, scale, p0, p1, x_dev, grad_dev, dx_dev) &
          bind(C, name="athena_mp_activation_param_bwd")
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr
       integer(c_int32_t), value :: kind
       integer(c_int64_t), value :: n
       real(c_float), value :: scale, p0, p1
       type(c_ptr), value :: x_dev, grad_dev, dx_dev
     end function

     !! ---- shaped activations and the concatenate merge ----
     integer(c_int) function athena_mp_swish_fwd(n, beta, x_dev, y_dev) bind(C, name="athena_mp_swish_fwd")
       import :: c_int, c_int64_t, c_float, c_ptr
       integer(c_int64_t), value :: n
       real(c_float), value :: beta
       type(c_ptr), value :: x_dev, y_dev
     end function
     integer(c_int) function athena_mp_swish_bwd(n, beta, x_dev, grad_dev, dx_dev) &
          bind(C, name="athena_mp_swish_bwd")
       import :: c_int, c_int64_t, c_float, c_ptr
       integer(c_int64_t), value :: n
       real(c_float), value :: beta
       type(c_ptr), value :: x_dev, grad_dev, dx_dev
     end function
     integer(c_int) function athena_mp_softmax_fwd(N, F, z_dev, y_dev) bind(C, name="athena_mp_softmax_fwd")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int64_t), value :: N
       integer(c_int32_t), value :: F
       type(c_ptr), value :: z_dev, y_dev
     end function
     integer(c_int) function athena_mp_softmax_bwd(N, F, y_dev, grad_dev, dz_dev) &
          bind(C, name="athena_mp_softmax_bwd")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int64_t), value :: N
       integer(c_int32_t), value :: F
       type(c_ptr), value :: y_dev, grad_dev, dz_dev
     end function
     integer(c_int) function athena_mp_concat_fwd(N, Fa, Fb, a_dev, b_dev, out_dev) &
          bind(C, name="athena_mp_concat_fwd")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int64_t), value :: N
       integer(c_int32_t), value :: Fa, Fb
       type(c_ptr), value :: a_dev, b_dev, out_dev
     end function
     integer(c_int) function athena_mp_concat_bwd(N, Fa, Fb, grad_dev, da_dev, db_dev) &
          bind(C, name="athena_mp_concat_bwd")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int64_t), value :: N
       integer(c_int32_t), value :: Fa, Fb
       type(c_ptr), value :: grad_dev, da_dev, db_dev
     end function

     !! ---- Duvenaud composite entry points (one launch each) ----
     integer(c_int) function athena_mp_duvenaud_update_act_fwd(graph, Fi, Fo, min_deg, max_deg, a_dev, &
          weight_dev, act, z_dev) bind(C, name="athena_mp_duvenaud_update_act_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, a_dev, weight_dev, z_dev
       integer(c_int32_t), value :: Fi, Fo, min_deg, max_deg, act
     end function
     integer(c_int) function athena_mp_duvenaud_readout_fwd(N, Fv, O, S, seg_dev, z_dev, R_dev, p_dev, &
          out_dev, accumulate) bind(C, name="athena_mp_duvenaud_readout_fwd")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int64_t), value :: N
       integer(c_int32_t), value :: Fv, O, S, accumulate
       type(c_ptr), value :: seg_dev, z_dev, R_dev, p_dev, out_dev
     end function
     integer(c_int) function athena_mp_duvenaud_readout_bwd(N, Fv, O, S, seg_dev, z_dev, R_dev, p_dev, &
          gout_dev, dz_next_dev, act, dc_dev, dR_dev, accumulate) bind(C, name="athena_mp_duvenaud_readout_bwd")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int64_t), value :: N
       integer(c_int32_t), value :: Fv, O, S, act, accumulate
       type(c_ptr), value :: seg_dev, z_dev, R_dev, p_dev, gout_dev, dz_next_dev, dc_dev, dR_dev
     end function

     !! ---- the remaining device-pointer entry points the layer types of athena_mp_layers use ----
     integer(c_int) function athena_mp_memset_zero(dev_ptr, bytes) bind(C, name="athena_mp_memset_zero")
       import :: c_int, c_ptr, c_int64_t
       type(c_ptr), value :: dev_ptr
       integer(c_int64_t), value :: bytes
     end function
     integer(c_int) function athena_mp_activation_fwd(act, n, z_dev, y_dev) bind(C, name="athena_mp_activation_fwd")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int32_t), value :: act
       integer(c_int64_t), value :: n
       type(c_ptr), value :: z_dev, y_dev
     end function
     integer(c_int) function athena_mp_device_copy(dst_dev, src_dev, bytes) bind(C, name="athena_mp_device_copy")
       import :: c_int, c_ptr, c_int64_t
       type(c_ptr), value :: dst_dev, src_dev
       integer(c_int64_t), value :: bytes
     end function
     integer(c_int) function athena_mp_axpy(n, alpha, x_dev, y_dev) bind(C, name="athena_mp_axpy")
       import :: c_int, c_int64_t, c_float, c_ptr
       integer(c_int64_t), value :: n
       real(c_float), value :: alpha
       type(c_ptr), value :: x_dev, y_dev
     end function
     !! y(:, v) = y(:, v) + b for the n_rows columns of y (f, n_rows): the bias of a layer whose dense step is no GEMM
     integer(c_int) function athena_mp_add_row_bias(n_rows, f, b_dev, y_dev) bind(C, name="athena_mp_add_row_bias")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int64_t), value :: n_rows
       integer(c_int32_t), value :: f
       type(c_ptr), value :: b_dev, y_dev
     end function
     integer(c_int) function athena_mp_kipf_propagate_act_fwd(graph, F, x_dev, act, y_dev) &
          bind(C, name="athena_mp_kipf_propagate_act_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, x_dev, y_dev
       integer(c_int32_t), value :: F, act
     end function
     integer(c_int) function athena_mp_kipf_propagate_bwd_dual(graph, F, g_dev, dx_plain_dev, dx_coef_dev) &
          bind(C, name="athena_mp_kipf_propagate_bwd_dual")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, g_dev, dx_plain_dev, dx_coef_dev
       integer(c_int32_t), value :: F
     end function
     integer(c_int) function athena_mp_duvenaud_propagate_fwd(graph, Fv, Fe, x_dev, e_dev, c_dev) &
          bind(C, name="athena_mp_duvenaud_propagate_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, x_dev, e_dev, c_dev
       integer(c_int32_t), value :: Fv, Fe
     end function
     integer(c_int) function athena_mp_duvenaud_propagate_bwd_x(graph, Fv, Fe, grad_dev, dx_dev) &
          bind(C, name="athena_mp_duvenaud_propagate_bwd_x")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, grad_dev, dx_dev
       integer(c_int32_t), value :: Fv, Fe
     end function
     integer(c_int) function athena_mp_duvenaud_propagate_bwd_e(graph, Fv, Fe, grad_dev, de_dev) &
          bind(C, name="athena_mp_duvenaud_propagate_bwd_e")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, grad_dev, de_dev
       integer(c_int32_t), value :: Fv, Fe
     end function
     integer(c_int) function athena_mp_duvenaud_update_bwd_a(graph, Fi, Fo, min_deg, max_deg, grad_dev, &
          weight_dev, da_dev) bind(C, name="athena_mp_duvenaud_update_bwd_a")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, grad_dev, weight_dev, da_dev
       integer(c_int32_t), value :: Fi, Fo, min_deg, max_deg
     end function
     integer(c_int) function athena_mp_duvenaud_update_bwd_w(graph, Fi, Fo, min_deg, max_deg, grad_dev, &
          a_dev, dweight_dev) bind(C, name="athena_mp_duvenaud_update_bwd_w")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, grad_dev, a_dev, dweight_dev
       integer(c_int32_t), value :: Fi, Fo, min_deg, max_deg
     end function
     !! update + activation + the readout's p = softmax(R z) in one launch (athena_duvenaud_msgpass_layer.f90:790-803,838-855)
     integer(c_int) function athena_mp_duvenaud_update_readout_fwd(graph, Fi, Fo, min_deg, max_deg, a_dev, weight_dev, act, &
          z_dev, O, R_dev, p_dev) bind(C, name="athena_mp_duvenaud_update_readout_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, a_dev, weight_dev, z_dev, R_dev, p_dev
       integer(c_int32_t), value :: Fi, Fo, min_deg, max_deg, act, O
     end function
     !! both partials of duvenaud_update from one pass over grad (:284-368)
     integer(c_int) function athena_mp_duvenaud_update_bwd(graph, Fi, Fo, min_deg, max_deg, grad_dev, a_dev, weight_dev, &
          da_dev, dweight_dev) bind(C, name="athena_mp_duvenaud_update_bwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, grad_dev, a_dev, weight_dev, da_dev, dweight_dev
       integer(c_int32_t), value :: Fi, Fo, min_deg, max_deg
     end function
     !! the same with da split where it is written: da_x (Fv, n) and da_e (Fe, n) instead of (Fv + Fe, n)
     integer(c_int) function athena_mp_duvenaud_update_bwd_split(graph, Fv, Fe, Fo, min_deg, max_deg, grad_dev, a_dev, weight_dev, &
          da_x_dev, da_e_dev, dweight_dev) bind(C, name="athena_mp_duvenaud_update_bwd_split")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, grad_dev, a_dev, weight_dev, da_x_dev, da_e_dev, dweight_dev
       integer(c_int32_t), value :: Fv, Fe, Fo, min_deg, max_deg
     end function
     !! one time step of the layer's reverse pass in one call: the readout's reverse (softmax -> matmul(R, z) -> activation) and
     !! the update's reverse, dc never in HBM where the shape allows it (Fv = 64, Fv + Fe <= 96, O <= 16)
     integer(c_int) function athena_mp_duvenaud_readout_update_bwd(graph, Fv, Fe, min_deg, max_deg, O, S, seg_dev, z_dev, R_dev, &
          p_dev, gout_dev, dz_next_dev, act, a_dev, weight_dev, da_x_dev, da_e_dev, dweight_dev, dR_dev, accumulate_dR, &
          accumulate_da_e, a_e_dev) bind(C, name="athena_mp_duvenaud_readout_update_bwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, seg_dev, z_dev, R_dev, p_dev, gout_dev, dz_next_dev, a_dev, weight_dev, da_x_dev, da_e_dev, &
            dweight_dev, dR_dev, a_e_dev
       integer(c_int32_t), value :: Fv, Fe, min_deg, max_deg, O, S, act, accumulate_dR, accumulate_da_e
     end function
     !! update + activation + the readout's p with a SPLIT: a_x (Fv, n) and a_e (Fe, n), the edge part gathered once per layer
     integer(c_int) function athena_mp_duvenaud_update_readout_fwd_split(graph, Fv, Fe, Fo, min_deg, max_deg, a_x_dev, a_e_dev, &
          weight_dev, act, z_dev, O, R_dev, p_dev) bind(C, name="athena_mp_duvenaud_update_readout_fwd_split")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, a_x_dev, a_e_dev, weight_dev, z_dev, R_dev, p_dev
       integer(c_int32_t), value :: Fv, Fe, Fo, min_deg, max_deg, act, O
     end function
     integer(c_int) function athena_mp_segment_sum(O, N, S, seg_dev, p_dev, out_dev, accumulate) &
          bind(C, name="athena_mp_segment_sum")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int32_t), value :: O, S, accumulate
       integer(c_int64_t), value :: N
       type(c_ptr), value :: seg_dev, p_dev, out_dev
     end function
     integer(c_int) function athena_mp_segment_sum_bwd(O, N, S, seg_dev, gout_dev, dp_dev) &
          bind(C, name="athena_mp_segment_sum_bwd")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       integer(c_int32_t), value :: O, S
       integer(c_int64_t), value :: N
       type(c_ptr), value :: seg_dev, gout_dev, dp_dev
     end function
     integer(c_int) function athena_mp_gno_aggregate_fwd(graph, d, H, Fi, Fo, theta_dev, coords_dev, x_dev, m_dev) &
          bind(C, name="athena_mp_gno_aggregate_fwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, theta_dev, coords_dev, x_dev, m_dev
       integer(c_int32_t), value :: d, H, Fi, Fo
     end function
     integer(c_int) function athena_mp_gno_aggregate_bwd_x(graph, d, H, Fi, Fo, theta_dev, coords_dev, grad_dev, &
          dx_dev) bind(C, name="athena_mp_gno_aggregate_bwd_x")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, theta_dev, coords_dev, grad_dev, dx_dev
       integer(c_int32_t), value :: d, H, Fi, Fo
     end function
     !! the same gradient as a PULL over the graph's own rows (row blocks of a partitioned undirected graph):
     !! dx [n_rows, Fi] from grad_ext [n_cols, Fo] -- athena_diffstruc_extd_sub_nop.f90:419-458 read from the receiving side
     integer(c_int) function athena_mp_gno_aggregate_bwd_x_pull(graph, d, H, Fi, Fo, theta_dev, coords_dev, grad_ext_dev, &
          dx_dev) bind(C, name="athena_mp_gno_aggregate_bwd_x_pull")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, theta_dev, coords_dev, grad_ext_dev, dx_dev
       integer(c_int32_t), value :: d, H, Fi, Fo
     end function
     !! the whole reverse pass of gno_aggregate from ONE G = g . Vmat^T: dx, dtheta and (on request) dcoords; any output
     !! may be c_null_ptr; s_save_dev = the S of athena_mp_gno_aggregate_fwd_save or c_null_ptr
     integer(c_int) function athena_mp_gno_aggregate_bwd(graph, d, H, Fi, Fo, theta_dev, coords_dev, x_dev, grad_dev, &
          s_save_dev, dx_dev, dtheta_dev, dcoords_dev, fused) bind(C, name="athena_mp_gno_aggregate_bwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, theta_dev, coords_dev, x_dev, grad_dev, s_save_dev, dx_dev, dtheta_dev, dcoords_dev
       integer(c_int32_t), value :: d, H, Fi, Fo
       integer(c_int32_t), intent(out) :: fused
     end function
     integer(c_int) function athena_mp_gno_aggregate_bwd_theta(graph, d, H, Fi, Fo, theta_dev, coords_dev, x_dev, &
          grad_dev, dtheta_dev) bind(C, name="athena_mp_gno_aggregate_bwd_theta")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, theta_dev, coords_dev, x_dev, grad_dev, dtheta_dev
       integer(c_int32_t), value :: d, H, Fi, Fo
     end function
     integer(c_int) function athena_mp_gno_aggregate_bwd_coords(graph, d, H, Fi, Fo, theta_dev, coords_dev, x_dev, &
          grad_dev, dcoords_dev) bind(C, name="athena_mp_gno_aggregate_bwd_coords")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, theta_dev, coords_dev, x_dev, grad_dev, dcoords_dev
       integer(c_int32_t), value :: d, H, Fi, Fo
     end function
     !! training-mode pair: the forward pass keeps S (bytes from _saved_bytes; 0 = shape not served) for dVaug = S^T g
     integer(c_int) function athena_mp_gno_saved_bytes(graph, d, H, Fi, Fo, bytes) bind(C, name="athena_mp_gno_saved_bytes")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value :: graph
       integer(c_int32_t), value :: d, H, Fi, Fo
       integer(c_int64_t), intent(out) :: bytes
     end function
     integer(c_int) function athena_mp_gno_aggregate_fwd_save(graph, d, H, Fi, Fo, theta_dev, coords_dev, x_dev, m_dev, &
          s_save_dev) bind(C, name="athena_mp_gno_aggregate_fwd_save")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, theta_dev, coords_dev, x_dev, m_dev, s_save_dev
       integer(c_int32_t), value :: d, H, Fi, Fo
     end function
     integer(c_int) function athena_mp_gno_aggregate_bwd_theta_saved(graph, d, H, Fi, Fo, theta_dev, coords_dev, x_dev, &
          grad_dev, s_save_dev, dtheta_dev) bind(C, name="athena_mp_gno_aggregate_bwd_theta_saved")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, theta_dev, coords_dev, x_dev, grad_dev, s_save_dev, dtheta_dev
       integer(c_int32_t), value :: d, H, Fi, Fo
     end function
     !! ---- multi-GPU (csrc/comm.hip): one process per GPU, RCCL over xGMI ------------------------------------------
     !! whole reverse pass of one step from its input X (no stored P): dX (may be c_null_ptr) and dW
     integer(c_int) function athena_mp_kipf_layer_bwd(graph, Fi, Fo, dZ_dev, W_dev, X_dev, exact, dX_dev, dW_dev) &
          bind(C, name="athena_mp_kipf_layer_bwd")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, dZ_dev, W_dev, X_dev, dX_dev, dW_dev
       integer(c_int32_t), value :: Fi, Fo, exact
     end function
     integer(c_int) function athena_mp_pull_gemm(graph, Fi, Fo, dZ_dev, W_dev, exact, dX_dev) &
          bind(C, name="athena_mp_pull_gemm")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: graph, dZ_dev, W_dev, dX_dev
       integer(c_int32_t), value :: Fi, Fo, exact
     end function
     integer(c_int) function athena_mp_comm_unique_id(id128) bind(C, name="athena_mp_comm_unique_id")
       import :: c_int, c_char
       character(kind=c_char), intent(inout) :: id128(128)
     end function
     integer(c_int) function athena_mp_comm_create(rank, world, id128, comm) bind(C, name="athena_mp_comm_create")
       import :: c_int, c_int32_t, c_char, c_ptr
       integer(c_int32_t), value :: rank, world
       character(kind=c_char), intent(in) :: id128(128)
       type(c_ptr), intent(out) :: comm
     end function
     integer(c_int) function athena_mp_comm_create_from_file(rank, world, path, comm) &
          bind(C, name="athena_mp_comm_create_from_file")
       import :: c_int, c_int32_t, c_char, c_ptr
       integer(c_int32_t), value :: rank, world
       character(kind=c_char), intent(in) :: path(*)     !! null-terminated
       type(c_ptr), intent(out) :: comm
     end function
     integer(c_int) function athena_mp_comm_destroy(comm) bind(C, name="athena_mp_comm_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: comm
     end function
     integer(c_int) function athena_mp_comm_barrier(comm) bind(C, name="athena_mp_comm_barrier")
       import :: c_int, c_ptr
       type(c_ptr), value :: comm
     end function
     integer(c_int) function athena_mp_allreduce(comm, buf_dev, count) bind(C, name="athena_mp_allreduce")
       import :: c_int, c_int64_t, c_ptr
       type(c_ptr), value :: comm, buf_dev
       integer(c_int64_t), value :: count
     end function
     integer(c_int) function athena_mp_allreduce_start(comm, buf_dev, count) bind(C, name="athena_mp_allreduce_start")
       import :: c_int, c_int64_t, c_ptr
       type(c_ptr), value :: comm, buf_dev
       integer(c_int64_t), value :: count
     end function
     integer(c_int) function athena_mp_allreduce_finish(comm) bind(C, name="athena_mp_allreduce_finish")
       import :: c_int, c_ptr
       type(c_ptr), value :: comm
     end function
     !! the rank's rows of graph_type%adj_ia / adj_ja (adj_ja(1,:) = GLOBAL neighbour ids)
     integer(c_int) function athena_mp_shard_create(comm, n_local, nnz, adj_ia, adj_ja, shard) &
          bind(C, name="athena_mp_shard_create")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value :: comm
       integer(c_int32_t), value :: n_local
       integer(c_int64_t), value :: nnz
       integer(c_int32_t), intent(in) :: adj_ia(*), adj_ja(2,*)
       type(c_ptr), intent(out) :: shard
     end function
     !! ... of a graph WITH edge features: adj_ja(2,:) = GLOBAL edge ids (0 = none); the shard's graphs keep the edge
     !! columns renumbered to the rank's own set (athena_mp_shard_export(7) lists their global ids)
     integer(c_int) function athena_mp_shard_create_edges(comm, n_local, nnz, adj_ia, adj_ja, shard) &
          bind(C, name="athena_mp_shard_create_edges")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value :: comm
       integer(c_int32_t), value :: n_local
       integer(c_int64_t), value :: nnz
       integer(c_int32_t), intent(in) :: adj_ia(*), adj_ja(2,*)
       type(c_ptr), intent(out) :: shard
     end function
     !! sum over the partition of a per-edge-column quantity (dcoords): cut columns exchanged with the peer that shares them
     integer(c_int) function athena_mp_shard_edge_reduce(shard, F, e_dev) bind(C, name="athena_mp_shard_edge_reduce")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: shard, e_dev
       integer(c_int32_t), value :: F
     end function
     integer(c_int) function athena_mp_shard_edge_cols(shard, n_edge_cols) bind(C, name="athena_mp_shard_edge_cols")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: shard
       integer(c_int32_t), intent(out) :: n_edge_cols
     end function
     integer(c_int) function athena_mp_shard_destroy(shard) bind(C, name="athena_mp_shard_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: shard
     end function
     integer(c_int) function athena_mp_shard_dims(shard, n_local, n_interior, n_halo, nnz, row_offset, n_total) &
          bind(C, name="athena_mp_shard_dims")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value :: shard
       integer(c_int32_t), intent(out) :: n_local, n_interior, n_halo
       integer(c_int64_t), intent(out) :: nnz, row_offset, n_total
     end function
     !! how the halo travels: mode 0 = grouped send / recv of packed rows, 1 = all-gather of whole blocks
     integer(c_int) function athena_mp_shard_info(shard, mode, fraction, tau, recv_rows) bind(C, name="athena_mp_shard_info")
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value :: shard
       integer(c_int32_t), intent(out) :: mode
       real(c_double), intent(out) :: fraction, tau
       integer(c_int64_t), intent(out) :: recv_rows
     end function
     integer(c_int) function athena_mp_shard_graph(shard, which, graph) bind(C, name="athena_mp_shard_graph")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: shard
       integer(c_int32_t), value :: which
       type(c_ptr), intent(out) :: graph
     end function
     integer(c_int) function athena_mp_shard_export(shard, which, host_dst, capacity, count) &
          bind(C, name="athena_mp_shard_export")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value :: shard
       integer(c_int32_t), value :: which
       type(*), dimension(*), intent(inout) :: host_dst
       integer(c_int64_t), value :: capacity
       integer(c_int64_t), intent(out) :: count
     end function
     !! the transpose of the exchange: rows computed for remote vertices (y_ext beyond the local rows) go to their owners and
     !! are added into y_local there -- the reverse pass of a partitioned graph in scatter form
     integer(c_int) function athena_mp_halo_reduce_start(shard, slot, F, y_ext_dev) bind(C, name="athena_mp_halo_reduce_start")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: shard, y_ext_dev
       integer(c_int32_t), value :: slot, F
     end function
     integer(c_int) function athena_mp_halo_reduce_finish(shard, slot, y_local_dev) bind(C, name="athena_mp_halo_reduce_finish")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: shard, y_local_dev
       integer(c_int32_t), value :: slot
     end function
     integer(c_int) function athena_mp_halo_start(shard, slot, F, x_ext_dev) bind(C, name="athena_mp_halo_start")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: shard, x_ext_dev
       integer(c_int32_t), value :: slot, F
     end function
     integer(c_int) function athena_mp_halo_finish(shard, slot) bind(C, name="athena_mp_halo_finish")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: shard
       integer(c_int32_t), value :: slot
     end function
  end interface

contains

  function athena_mp_dev_offset(p, elements) result(q)
    !! device pointer `elements` float32 values past p (row blocks of a resident tensor)
    type(c_ptr), intent(in) :: p
    integer(c_int64_t), intent(in) :: elements
    type(c_ptr) :: q
    q = transfer(transfer(p, 0_c_intptr_t) + 4_c_intptr_t * int(elements, c_intptr_t), q)
  end function athena_mp_dev_offset

  function athena_mp_error_message() result(msg)
    !! last C-side error as a Fortran string (what the layer hands to coreutils' stop_program)
    character(len=:), allocatable :: msg
    type(c_ptr) :: p
    character(kind=c_char), pointer :: s(:)
    integer :: n
    p = athena_mp_last_error()
    if(.not.c_associated(p))then
       msg = ""
       return
    end if
    call c_f_pointer(p, s, [1024])
    n = 0
    do while(n .lt. 1024)
       if(s(n+1) .eq. c_null_char) exit
       n = n + 1
    end do
    allocate(character(len=n) :: msg)
    msg = transfer(s(1:n), msg)
  end function athena_mp_error_message

end module athena_mp_c
