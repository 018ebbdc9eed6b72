!! Max pooling between TWO point sets from FORTRAN through the C ABI, with its reverse steps: what a caller that holds Fortran
!! arrays does for the set-abstraction step of a multi-scale operator -- the k-nearest-neighbour graph of the coarse points in the
!! fine ones, the handle from that CSR, the maximum over each neighbourhood of per-vertex and of per-edge values with its arg-max,
!! and both gradients.
!!
!!   pool_run <case-file> <result-file>
!!
!! case file (stream):   int32 n_queries, n_sources, dim, k, F; real32 radius (ieee +infinity: no cap);
!!                       real32 queries(dim, n_queries), sources(dim, n_sources), x(F, n_sources), h(F, n_queries * k),
!!                       dy(F, n_queries)
!!                       (h holds a row for every pair the graph can have; the first `pairs` of them are the edge values)
!! result file (stream): int64 pairs; real32 y_x(F, n_queries); int32 arg_x(F, n_queries); real32 y_h(F, n_queries);
!!                       int32 arg_h(F, n_queries); real32 dx(F, n_sources), dh(F, pairs)
!! tests/test_gpu_pool.py compares the arrays with the device entries' bytes.
program pool_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit, i
  integer(c_int32_t) :: nq, ns, dim, k, F
  integer(c_int32_t) :: query_offsets(2), source_offsets(2)
  real(c_float) :: radius
  real(c_float), allocatable :: queries(:,:), sources(:,:), dy(:,:)
  real(c_float), allocatable, target :: x(:,:), h(:,:)
  integer(c_int32_t), allocatable, target :: adj_ia(:), adj_ja(:,:), row_deg(:), col_deg(:), arg_x(:,:), arg_h(:,:)
  real(c_float), allocatable, target :: coords(:,:), y_x(:,:), y_h(:,:), dx(:,:), dh(:,:)
  integer(c_int64_t) :: pairs
  type(c_ptr) :: graph

  if(command_argument_count() .lt. 2) stop "usage: pool_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) nq, ns, dim, k, F
  read(unit) radius
  allocate(queries(dim, nq), sources(dim, ns), x(F, ns), h(F, nq * k), dy(F, nq))
  read(unit) queries, sources, x, h, dy
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

  ! fine to coarse over the vertices' and over the edges' values, and back
  allocate(y_x(F, nq), arg_x(F, nq), y_h(F, nq), arg_h(F, nq), dx(F, ns), dh(F, pairs))
  call must(athena_mp_pool_max_host(graph, F, c_loc(x), c_null_ptr, y_x, c_loc(arg_x)), "pool_max_host (x)")
  call must(athena_mp_pool_max_host(graph, F, c_null_ptr, c_loc(h), y_h, c_loc(arg_h)), "pool_max_host (h)")
  call must(athena_mp_pool_max_bwd_host(graph, F, arg_x, dy, c_loc(dx), c_null_ptr), "pool_max_bwd_host (dx)")
  call must(athena_mp_pool_max_bwd_host(graph, F, arg_h, dy, c_null_ptr, c_loc(dh)), "pool_max_bwd_host (dh)")
  call must(athena_mp_graph_destroy(graph), "graph_destroy")

  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  write(unit) pairs
  write(unit) y_x, arg_x, y_h, arg_h, dx, dh
  close(unit)
  write(*,'(A,I0,A,I0,A,I0,A,I0,A)') "max pooling: ", nq, " queries, ", ns, " sources, ", pairs, " pairs, ", F, " features"
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
end program pool_run
