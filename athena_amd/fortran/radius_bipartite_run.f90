!! The radius graph between TWO point sets from FORTRAN through the C ABI, and its gradient back to both sets: what a caller that
!! holds Fortran arrays does around graph_nop_layer_type on a rectangular graph (a mesh onto a latent grid, a grid onto query
!! points) -- query, allocate, fill; then the handle from that CSR, and the reverse step on it.
!!
!!   radius_bipartite_run <case-file> <result-file>
!!
!! case file (stream):   int32 n_clouds, n_queries, n_sources, dim; real32 radius; int32 query_offsets(n_clouds + 1),
!!                       source_offsets(n_clouds + 1); real32 queries(dim, n_queries), sources(dim, n_sources);
!!                       int64 pairs; real32 dcoords(dim, pairs)
!! result file (stream): int64 pairs; int32 adj_ia(n_queries + 1), adj_ja(2, pairs); real32 coords(dim, pairs);
!!                       int64 edge_offsets(n_clouds + 1); real32 dqueries(dim, n_queries), dsources(dim, n_sources)
!! tests/test_gpu_radius_bipartite.py compares the arrays with the yardstick's.
program radius_bipartite_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit, i
  integer(c_int32_t) :: n_clouds, nq, ns, dim
  real(c_float) :: radius
  integer(c_int32_t), allocatable :: query_offsets(:), source_offsets(:)
  real(c_float), allocatable :: queries(:,:), sources(:,:), dcoords(:,:)
  integer(c_int32_t), allocatable, target :: adj_ia(:), adj_ja(:,:), row_deg(:), col_deg(:)
  real(c_float), allocatable, target :: coords(:,:), dqueries(:,:), dsources(:,:)
  integer(c_int64_t), allocatable, target :: edge_offsets(:)
  integer(c_int64_t) :: pairs, pairs_given
  type(c_ptr) :: graph

  if(command_argument_count() .lt. 2) stop "usage: radius_bipartite_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) n_clouds, nq, ns, dim
  read(unit) radius
  allocate(query_offsets(n_clouds + 1), source_offsets(n_clouds + 1), queries(dim, nq), sources(dim, ns), edge_offsets(n_clouds + 1))
  read(unit) query_offsets, source_offsets
  read(unit) queries, sources
  read(unit) pairs_given
  allocate(dcoords(dim, pairs_given))
  read(unit) dcoords
  close(unit)

  call must(athena_mp_init(0_c_int), "init")
  ! case 1: the search through the host form
  call must(athena_mp_radius_graph_bipartite_host(n_clouds, nq, query_offsets, ns, source_offsets, dim, queries, sources, radius, &
       c_null_ptr, c_null_ptr, 0_c_int64_t, c_null_ptr, 0_c_int64_t, c_null_ptr, pairs), "radius_graph_bipartite_host (size query)")
  if(pairs .ne. pairs_given) stop "the case file's dcoords do not fit the graph"
  allocate(adj_ia(nq + 1), adj_ja(2, pairs), coords(dim, pairs))
  call must(athena_mp_radius_graph_bipartite_host(n_clouds, nq, query_offsets, ns, source_offsets, dim, queries, sources, radius, &
       c_loc(adj_ia), c_loc(adj_ja), pairs, c_loc(coords), pairs, c_loc(edge_offsets), pairs), "radius_graph_bipartite_host")

  ! case 2: the handle from that CSR (degrees = row and column lengths) and the gradient back to both sets
  allocate(row_deg(nq), col_deg(ns), dqueries(dim, nq), dsources(dim, ns))
  row_deg = adj_ia(2:nq + 1) - adj_ia(1:nq)
  col_deg = 0
  do i = 1, int(pairs)
     col_deg(adj_ja(1, i)) = col_deg(adj_ja(1, i)) + 1
  end do
  call must(athena_mp_graph_create(nq, ns, pairs, adj_ia, adj_ja, int(pairs, c_int32_t), c_loc(row_deg), c_loc(col_deg), graph), &
       "graph_create")
  call must(athena_mp_edge_grad_to_point_sets_host(graph, dim, dcoords, c_loc(dqueries), c_loc(dsources)), &
       "edge_grad_to_point_sets_host")
  call must(athena_mp_graph_destroy(graph), "graph_destroy")

  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  write(unit) pairs
  write(unit) adj_ia, adj_ja, coords, edge_offsets, dqueries, dsources
  close(unit)
  write(*,'(A,I0,A,I0,A,I0,A,I0,A)') "two-set radius graph: ", n_clouds, " clouds, ", nq, " queries, ", ns, " sources, ", pairs, " pairs"
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
end program radius_bipartite_run
