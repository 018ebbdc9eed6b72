!! Inverse-distance interpolation between TWO point sets from FORTRAN through the C ABI, with its gradients: what a caller that
!! holds Fortran arrays does for the coarse-to-fine step of a multi-scale operator -- the k-nearest-neighbour graph of the fine
!! points in the coarse ones, the handle from that CSR, the interpolated features, and the reverse step down to both point sets.
!!
!!   interp_run <case-file> <result-file>
!!
!! case file (stream):   int32 n_queries, n_sources, dim, k, F; real32 radius (ieee +infinity: no cap), eps;
!!                       real32 queries(dim, n_queries), sources(dim, n_sources), x(F, n_sources), dy(F, n_queries)
!! result file (stream): int64 pairs; real32 coords(dim, pairs), weights(pairs), y(F, n_queries), dx(F, n_sources),
!!                       dcoords(dim, pairs), dqueries(dim, n_queries), dsources(dim, n_sources)
!! tests/test_gpu_interp.py compares the arrays with the device entries' bytes.
program interp_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit, i
  integer(c_int32_t) :: nq, ns, dim, k, F
  integer(c_int32_t) :: query_offsets(2), source_offsets(2)
  real(c_float) :: radius, eps
  real(c_float), allocatable :: queries(:,:), sources(:,:), x(:,:), dy(:,:)
  integer(c_int32_t), allocatable, target :: adj_ia(:), adj_ja(:,:), row_deg(:), col_deg(:)
  real(c_float), allocatable, target :: coords(:,:), weights(:), y(:,:), dx(:,:), dcoords(:,:), dqueries(:,:), dsources(:,:)
  integer(c_int64_t) :: pairs
  type(c_ptr) :: graph

  if(command_argument_count() .lt. 2) stop "usage: interp_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) nq, ns, dim, k, F
  read(unit) radius, eps
  allocate(queries(dim, nq), sources(dim, ns), x(F, ns), dy(F, nq))
  read(unit) queries, sources, x, dy
  close(unit)
  query_offsets = [0_c_int32_t, nq]
  source_offsets = [0_c_int32_t, ns]

  call must(athena_mp_init(0_c_int), "init")
  ! the graph: query, allocate, fill
  call must(athena_mp_knn_graph_bipartite_host(1_c_int32_t, nq, query_offsets, ns, source_offsets, dim, queries, sources, k, radius, &
       c_null_ptr, c_null_ptr, 0_c_int64_t, c_null_ptr, 0_c_int64_t, c_null_ptr, c_null_ptr, c_null_ptr, pairs), &
       "knn_graph_bipartite_host (size query)")
  allocate(adj_ia(nq + 1), adj_ja(2, pairs), coords(dim, pairs))
  call must(athena_mp_knn_graph_bipartite_host(1_c_int32_t, nq, query_offsets, ns, source_offsets, dim, queries, sources, k, radius, &
       c_loc(adj_ia), c_loc(adj_ja), pairs, c_loc(coords), pairs, c_null_ptr, c_null_ptr, c_null_ptr, pairs), &
       "knn_graph_bipartite_host")
  allocate(row_deg(nq), col_deg(ns))
  row_deg = adj_ia(2:nq + 1) - adj_ia(1:nq)
  col_deg = 0
  do i = 1, int(pairs)
     col_deg(adj_ja(1, i)) = col_deg(adj_ja(1, i)) + 1
  end do
  call must(athena_mp_graph_create(nq, ns, pairs, adj_ia, adj_ja, int(pairs, c_int32_t), c_loc(row_deg), c_loc(col_deg), graph), &
       "graph_create")

  ! coarse to fine, and back
  allocate(weights(pairs), y(F, nq), dx(F, ns), dcoords(dim, pairs), dqueries(dim, nq), dsources(dim, ns))
  call must(athena_mp_interp_host(graph, dim, F, coords, eps, x, y, c_loc(weights)), "interp_host")
  call must(athena_mp_interp_bwd_host(graph, dim, F, coords, eps, x, dy, c_loc(dx), c_loc(dcoords)), "interp_bwd_host")
  call must(athena_mp_edge_grad_to_point_sets_host(graph, dim, dcoords, c_loc(dqueries), c_loc(dsources)), &
       "edge_grad_to_point_sets_host")
  call must(athena_mp_graph_destroy(graph), "graph_destroy")

  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  write(unit) pairs
  write(unit) coords, weights, y, dx, dcoords, dqueries, dsources
  close(unit)
  write(*,'(A,I0,A,I0,A,I0,A,I0,A)') "interpolation: ", nq, " queries, ", ns, " sources, ", pairs, " pairs, ", F, " features"
  call must(athena_mp_finalize(), "finalize")

contains

  subroutine must(rc, what)
    integer(c_int), intent(in) :: rc
    character(*), intent(in) :: what
    if(rc .ne. 0)then
       write(0,*) what//" failed: "//athena_mp_error_message()
       stop 1
    end if
  end subroutine must
end program interp_run
