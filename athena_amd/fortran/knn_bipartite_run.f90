!! The k-nearest-neighbour graph between TWO point sets from FORTRAN through the C ABI: what a caller that holds Fortran arrays
!! does in front of graph_nop_layer_type on a rectangular graph whose queries may lie anywhere -- query, allocate, fill.
!!
!!   knn_bipartite_run <case-file> <result-file>
!!
!! case file (stream):   int32 n_clouds, n_queries, n_sources, dim, k; real32 radius (ieee +infinity: no cap);
!!                       int32 query_offsets(n_clouds + 1), source_offsets(n_clouds + 1);
!!                       real32 queries(dim, n_queries), sources(dim, n_sources)
!! result file (stream): int64 pairs; int32 adj_ia(n_queries + 1), adj_ja(2, pairs); real32 coords(dim, pairs);
!!                       int64 edge_offsets(n_clouds + 1); int32 nbr(k, n_queries); real32 sqdist(k, n_queries)
!! tests/test_gpu_knn_bipartite.py compares the arrays with the yardstick's.
program knn_bipartite_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit
  integer(c_int32_t) :: n_clouds, nq, ns, dim, k
  real(c_float) :: radius
  integer(c_int32_t), allocatable :: query_offsets(:), source_offsets(:)
  real(c_float), allocatable :: queries(:,:), sources(:,:)
  integer(c_int32_t), allocatable, target :: adj_ia(:), adj_ja(:,:), nbr(:,:)
  real(c_float), allocatable, target :: coords(:,:), sqdist(:,:)
  integer(c_int64_t), allocatable, target :: edge_offsets(:)
  integer(c_int64_t) :: pairs, pairs_again

  if(command_argument_count() .lt. 2) stop "usage: knn_bipartite_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) n_clouds, nq, ns, dim, k
  read(unit) radius
  allocate(query_offsets(n_clouds + 1), source_offsets(n_clouds + 1), queries(dim, nq), sources(dim, ns), edge_offsets(n_clouds + 1))
  read(unit) query_offsets, source_offsets
  read(unit) queries, sources
  close(unit)

  call must(athena_mp_init(0_c_int), "init")
  call must(athena_mp_knn_graph_bipartite_host(n_clouds, nq, query_offsets, ns, source_offsets, dim, queries, sources, k, radius, &
       c_null_ptr, c_null_ptr, 0_c_int64_t, c_null_ptr, 0_c_int64_t, c_null_ptr, c_null_ptr, c_null_ptr, pairs), &
       "knn_graph_bipartite_host (size query)")
  allocate(adj_ia(nq + 1), adj_ja(2, pairs), coords(dim, pairs), nbr(k, nq), sqdist(k, nq))
  call must(athena_mp_knn_graph_bipartite_host(n_clouds, nq, query_offsets, ns, source_offsets, dim, queries, sources, k, radius, &
       c_loc(adj_ia), c_loc(adj_ja), pairs, c_loc(coords), pairs, c_loc(nbr), c_loc(sqdist), c_loc(edge_offsets), pairs_again), &
       "knn_graph_bipartite_host")
  if(pairs_again .ne. pairs) stop "the size query and the fill disagree"

  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  write(unit) pairs
  write(unit) adj_ia, adj_ja, coords, edge_offsets, nbr, sqdist
  close(unit)
  write(*,'(A,I0,A,I0,A,I0,A,I0,A,I0,A)') "two-set k-nearest-neighbour graph: ", n_clouds, " clouds, ", nq, " queries, ", ns, &
       " sources, k = ", k, ", ", pairs, " pairs"
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
end program knn_bipartite_run
