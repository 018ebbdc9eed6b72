!! Bond-angle triplets of a radius graph from FORTRAN through the C ABI, with the gradient back to the edge vectors: what a caller
!! that holds Fortran arrays does for a three-body term -- the radius graph of the points, the handle from that CSR, the triplet CSR
!! with the entry vectors and the cosines (query, allocate, fill), and dcos -> dvec in one call.
!!
!!   triplets_run <case-file> <result-file>
!!
!! case file (stream):   int32 n, dim, add_self_loops; real32 radius, cutoff3 (ieee +infinity: every entry);
!!                       int64 n_dcos; real32 points(dim, n), dcos(n_dcos)
!!                       (dcos holds a value for every triplet the graph can have; the first `triplets` of them are used)
!! result file (stream): int64 pairs, nnz, triplets; int32 adj_ia(nnz + 1), adj_ja(2, triplets); real32 dir(dim, nnz),
!!                       cos(triplets), dvec(dim, pairs)
!! tests/test_gpu_triplets.py compares the arrays with the Python mirror's.
program triplets_run
  use, intrinsic :: iso_c_binding
  use athena_mp_c
  implicit none
  character(1024) :: case_file, result_file
  integer :: unit
  integer(c_int32_t) :: n, dim, loops
  real(c_float) :: radius, cutoff3
  real(c_float), allocatable :: points(:,:), dcos(:)
  integer(c_int32_t), allocatable, target :: adj_ia(:), adj_ja(:,:), t_ia(:), t_ja(:,:)
  real(c_float), allocatable, target :: coords(:,:), dir(:,:), cosv(:), dvec(:,:)
  integer(c_int64_t) :: nnz, pairs, triplets, n_dcos
  type(c_ptr) :: graph

  if(command_argument_count() .lt. 2) stop "usage: triplets_run case-file result-file"
  call get_command_argument(1, case_file)
  call get_command_argument(2, result_file)
  open(newunit=unit, file=trim(case_file), access="stream", form="unformatted", status="old")
  read(unit) n, dim, loops
  read(unit) radius, cutoff3
  read(unit) n_dcos
  allocate(points(dim, n), dcos(n_dcos))
  read(unit) points, dcos
  close(unit)

  call must(athena_mp_init(0_c_int), "init")
  ! the graph: query, allocate, fill; then its handle, with one edge column per pair
  call must(athena_mp_radius_graph_host(n, dim, points, radius, loops, c_null_ptr, c_null_ptr, 0_c_int64_t, nnz, &
       c_null_ptr, 0_c_int64_t, pairs), "radius_graph_host (size query)")
  allocate(adj_ia(n + 1), adj_ja(2, nnz), coords(dim, pairs))
  call must(athena_mp_radius_graph_host(n, dim, points, radius, loops, c_loc(adj_ia), c_loc(adj_ja), nnz, nnz, &
       c_loc(coords), pairs, pairs), "radius_graph_host")
  call must(athena_mp_graph_create(n, n, nnz, adj_ia, adj_ja, int(pairs, c_int32_t), c_null_ptr, c_null_ptr, graph), "graph_create")

  ! the triplets: query, allocate, fill
  call must(athena_mp_triplets_host(graph, dim, c_loc(coords), cutoff3, c_null_ptr, c_null_ptr, 0_c_int64_t, c_null_ptr, c_null_ptr, &
       triplets), "triplets_host (size query)")
  if(triplets .gt. n_dcos) stop "the case file holds fewer dcos values than the graph has triplets"
  allocate(t_ia(nnz + 1), t_ja(2, triplets), dir(dim, nnz), cosv(triplets), dvec(dim, pairs))
  call must(athena_mp_triplets_host(graph, dim, c_loc(coords), cutoff3, c_loc(t_ia), c_loc(t_ja), triplets, c_loc(dir), c_loc(cosv), &
       triplets), "triplets_host")
  ! ... and the gradient per triplet back to the edge vectors
  call must(athena_mp_triplet_cos_bwd_host(graph, dim, coords, cutoff3, triplets, dcos, dvec), "triplet_cos_bwd_host")
  call must(athena_mp_graph_destroy(graph), "graph_destroy")

  open(newunit=unit, file=trim(result_file), access="stream", form="unformatted", status="replace")
  write(unit) pairs, nnz, triplets
  write(unit) t_ia, t_ja, dir, cosv, dvec
  close(unit)
  write(*,'(A,I0,A,I0,A,I0,A,I0,A)') "triplets: ", n, " points, ", pairs, " pairs, ", nnz, " entries, ", triplets, " triplets"
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
end program triplets_run
